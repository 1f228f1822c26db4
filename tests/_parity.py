"""Parity checks shared by the CPU (host-emulation build) and GPU (product build) suites.
The library under test is driven through the C ABI; the oracle / golden fixtures check it."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla
from scipy.sparse import csr_matrix as sps_csr

import porepy_amd as pa
from oracle import mpfa_oracle as mo
from tests._golden import SubfaceCase, BIOT_KEYS, BiotCase, MPSA_KEYS, MpsaPartialCase, ALL_KEYS, Case, PartialCase, TiltedCase, check_pattern, rel_max_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_SO = os.path.join(ROOT, "oracle", "_build", "libporefv_emul.so")
TOL = 1e-10  # north_star: matrix entries and fields within 1e-10 relative
# Delaunay SLIVER fixtures (cells of aspect ratio ~1e4): the condensed local systems carry coefficients nK D^-1 of
# size cond(D); after iterative refinement what is left is the sensitivity of the result to the ROUNDING of those
# coefficients, ~1e6 eps here -- 2e-11 on the host build, 1.3e-10 on the device (different contraction of the same
# sums): both are draws from that distribution.  Without the refinement the same cases are off by 3e-8..2e-6.
SLIVER_TOL = 1e-9


def tol_for(name: str) -> float:
    return SLIVER_TOL if "sliver" in name else TOL

WHICH = dict(zip(ALL_KEYS, range(6)))


def emulation_library():
    """Host-emulation build of porepy_amd/csrc (same kernel sources, sequential lanes)."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    if ge._stale(EMUL_SO):
        os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
        subprocess.run(["g++", "-x", "c++", "-DPFV_EMULATE", "-O2", "-std=c++17", "-shared", "-fPIC",
                        "-Wno-maybe-uninitialized", "porefv.hip", "-o", EMUL_SO],
                       check=True, cwd=os.path.join(ROOT, "porepy_amd", "csrc"))
    return pa._lib.load_library(EMUL_SO)


def dropin_library():
    """Library under the reference's models in tests/_dropin_*_script.py: the host emulation in the build
    container (no GPU), the PRODUCT library (libporefv_hip.so) when PFV_DROPIN_LIBRARY=product (-m gpu)."""
    if os.environ.get("PFV_DROPIN_LIBRARY", "emulation") == "product":
        return pa._lib.product_library()
    return emulation_library()


def flags_of(bc: dict) -> np.ndarray:
    return (bc["is_dir"] * 1 + bc["is_neu"] * 2 + bc["is_rob"] * 4 + bc["is_internal"] * 8).astype(np.uint8)


def run_case(lib, c: Case):
    ctx = pa.Context(0, lib)
    ctx.set_grid(c.grid)
    eta = c.eta if c.eta is not None else mo.default_eta(c.grid["name"])
    ctx.set_params(c.perm, flags_of(c.bc), c.bc["robin_weight"], eta, getattr(c, "eta_sub", None))
    ctx.discretize()
    return ctx


def check_golden_case(lib, name: str):
    c = Case(name)
    TOL = tol_for(name)  # noqa: N806
    ctx = run_case(lib, c)
    ora = mo.discretize(c.grid, c.perm, c.bc, eta=c.eta_sub if c.eta_sub is not None else c.eta)
    for k in ALL_KEYS:
        M = ctx.matrix(WHICH[k])
        assert M.indices.dtype == np.int32 and M.has_sorted_indices
        # pattern: bit-exact against the oracle's structural stencil
        assert np.array_equal(M.indptr, ora[k].indptr), (name, k)
        assert np.array_equal(M.indices, ora[k].indices), (name, k)
        assert rel_max_err(M, ora[k]) < TOL, (name, k)
        if k in c.ref:  # and against what the reference itself produced
            assert rel_max_err(M, c.ref[k]) < TOL, (name, k)
            subset, outside, _ = check_pattern(M, c.ref[k])
            assert subset and outside < 1e-12, (name, k, outside)
    ctx.assemble(c.bc_values, c.vector_source_values, c.source)
    A, b = ctx.matrix(6), ctx.rhs()
    assert rel_max_err(A, c.ref["A"]) < TOL
    assert np.linalg.norm(b - c.ref_rhs) <= TOL * np.linalg.norm(c.ref_rhs)
    x, info = ctx.solve("bicgstab", rtol=1e-13, maxit=5000)
    assert info["converged"]
    # field: residual in the REFERENCE system, and the field itself where A is well conditioned
    res = np.linalg.norm(c.ref_rhs - c.ref["A"] @ x) / np.linalg.norm(c.ref_rhs)
    # (sliver grids: the system matrix is ill conditioned, a 1e-11 difference in its entries shows in the residual)
    assert res < (1e-8 if "sliver" in name else 1e-11), (name, res)
    if "hetero" not in name and "sliver" not in name:
        assert np.linalg.norm(x - c.ref_x) <= TOL * np.linalg.norm(c.ref_x), name
    # flux post-processing through the device SpMV
    fl = ctx.spmv(0, x) + ctx.spmv(1, c.bc_values)
    fl_ref = c.ref["flux"] @ c.ref_x + c.ref["bound_flux"] @ c.bc_values
    assert np.linalg.norm(fl - fl_ref) <= (1e-6 if "sliver" in name else 1e-9) * max(np.linalg.norm(fl_ref), 1e-300)
    ctx.close()


def check_generic_pattern_bit_exact(lib):
    c = Case("tet_2x2x2_dir_generic")
    ctx = run_case(lib, c)
    for k in ("flux", "bound_flux", "vector_source"):
        M = ctx.matrix(WHICH[k])
        assert np.array_equal(M.indptr, c.ref[k].indptr), k
        assert np.array_equal(M.indices, c.ref[k].indices), k
    ctx.assemble(c.bc_values, None, c.source)
    A = ctx.matrix(6)
    assert np.array_equal(A.indptr, c.ref["A"].indptr) and np.array_equal(A.indices, c.ref["A"].indices)


def check_known_answer(lib, key: str):
    """The reference's own golden vectors (tests/numerics/fv/test_mpfa.py:224-250)."""
    c = Case("known_" + key)
    ctx = run_case(lib, c)
    ctx.assemble(c.bc_values, None, c.source)
    u, info = ctx.solve("bicgstab", rtol=1e-13, maxit=5000)
    flux = ctx.spmv(0, u) + ctx.spmv(1, c.bc_values)
    assert np.allclose(u, c.known_u)
    assert np.allclose(flux, c.known_flux)


def operator_roundtrip(lib, g, seed=0, kinds=("dir", "neu", "rob"), hetero=1.0):
    """Mpfa operator API on one of this package's grids, compared with the oracle."""
    rng = np.random.default_rng(seed)
    nc = g.num_cells
    kk = np.where(g.cell_centers[0] > 0.5 * g.nodes[0].max(), hetero, 1.0)
    kw = dict(kxx=kk * (1 + rng.random(nc)), kyy=kk * (2 + rng.random(nc)), kxy=kk * 0.3 * rng.random(nc))
    if g.dim == 3:
        kw.update(kzz=kk * (0.5 + rng.random(nc)), kxz=kk * 0.1 * rng.random(nc), kyz=kk * 0.1 * rng.random(nc))
    K = pa.SecondOrderTensor(**kw)
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, list(np.array(kinds)[np.arange(bf.size) % len(kinds)]))
    bc.robin_weight = 0.7 + rng.random(g.num_faces)
    bv = np.zeros(g.num_faces)
    bv[bf] = rng.random(bf.size) - 0.4
    gv = rng.random(nc * g.dim) - 0.5
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "bc_values": bv,
                                           "vector_source": gv})
    discr = pa.Mpfa("flow", library=lib)
    discr.discretize(g, data)
    raw = pa.grid_to_raw(g)
    ora = mo.discretize(raw, K.values, pa.bc_to_raw(bc))
    mats = data[pa.DISCRETIZATION_MATRICES]["flow"]
    for k in ALL_KEYS:
        assert np.array_equal(mats[k].indices, ora[k].indices), k
        assert rel_max_err(mats[k], ora[k]) < TOL, k
    A, b = discr.assemble_matrix_rhs(g, data)
    Ao, bo = mo.assemble_matrix_rhs(raw, ora, bv, gv)
    assert rel_max_err(A, Ao) < TOL
    assert np.linalg.norm(b - bo) <= TOL * np.linalg.norm(bo)
    src = rng.random(nc) * g.cell_volumes
    x, info = discr.solve(g, data, source=src, rtol=1e-13)
    xo = spla.spsolve(Ao.tocsc(), bo + src)
    assert np.linalg.norm(bo + src - Ao @ x) <= 1e-11 * np.linalg.norm(bo + src)
    if hetero == 1.0:
        assert np.linalg.norm(x - xo) <= TOL * np.linalg.norm(xo)
    return discr, data


class _RawBC:
    """Boundary-condition holder filled from fixture arrays."""

    def __init__(self, raw):
        for k, v in raw.items():
            setattr(self, k, v)


def check_partial_case(lib, name: str):
    """specified_cells / _faces / _nodes and update_discretization against what the reference
    produced (oracle/gen_golden_partial.py; semantics of tests/numerics/fv/test_mpfa.py:503-640)."""
    c = PartialCase(name)
    g = pa.grid_from_raw(c.grid)
    bc = _RawBC(c.bc)
    K = type("K", (), {"values": c.perm})()
    full = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc})
    d_full = pa.Mpfa("flow", library=lib)
    d_full.discretize(g, full)
    full_m = full[pa.DISCRETIZATION_MATRICES]["flow"]
    for sub in c.partial:
        data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, **sub["spec"]})
        d = pa.Mpfa("flow", library=lib)
        d.discretize(g, data)
        pd = data[pa.PARAMETERS]["flow"]
        assert np.array_equal(pd["active_faces"], sub["active_faces"]), (name, sub["spec"])
        assert np.array_equal(pd["active_cells"], np.unique(sub["active_cells"])), (name, sub["spec"])
        af = sub["active_faces"]
        inactive = np.setdiff1d(np.arange(g.num_faces), af)
        for k in ALL_KEYS:
            M = data[pa.DISCRETIZATION_MATRICES]["flow"][k]
            assert M.shape == sub["mats"][k].shape
            assert rel_max_err(M, sub["mats"][k]) < TOL, (name, sub["spec"], k)
            assert M[inactive].nnz == 0, (name, k)           # only the active rows are filled
            assert rel_max_err(M[af], full_m[k][af]) < TOL   # and they are the full discretization's rows
    # update: new permeability in a few cells, every other row kept on the device
    Knew = type("K", (), {"values": c.perm_new})()
    full[pa.PARAMETERS]["flow"]["second_order_tensor"] = Knew
    full["update_discretization"] = {"modified_cells": c.modified_cells}
    d_full.update_discretization(g, full)
    fresh = pa.initialize_data({}, "flow", {"second_order_tensor": Knew, "bc": bc})
    pa.Mpfa("flow", library=lib).discretize(g, fresh)
    for k in ALL_KEYS:
        M = full[pa.DISCRETIZATION_MATRICES]["flow"][k]
        assert rel_max_err(M, c.updated[k]) < TOL, (name, "update", k)
        assert rel_max_err(M, fresh[pa.DISCRETIZATION_MATRICES]["flow"][k]) < TOL
    # ... and the rows away from the modified cells were not touched (bit-identical)
    _, touched = pa.active_indices(g, cells=c.modified_cells)
    untouched = np.setdiff1d(np.arange(g.num_faces), touched)
    assert untouched.size > 0
    assert np.array_equal(full[pa.DISCRETIZATION_MATRICES]["flow"]["flux"][untouched].data,
                          full_m["flux"][untouched].data)


def check_tilted_case(lib, name: str):
    """2-D grid rotated out of the xy-plane, full 3-D permeability, 3-D vector source:
    every matrix, A and b against the reference (mpfa.py:733-754, 422-463)."""
    c = TiltedCase(name)
    g = pa.grid_from_raw(c.grid)
    K = type("K", (), {"values": c.perm})()
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": _RawBC(c.bc), "bc_values": c.bc_values,
                                           "ambient_dimension": c.vdim, "vector_source": c.vector_source_values})
    d = pa.Mpfa("flow", library=lib)
    d.discretize(g, data)
    for k in ALL_KEYS:
        M = data[pa.DISCRETIZATION_MATRICES]["flow"][k]
        assert M.shape == c.ref[k].shape, (name, k)
        assert rel_max_err(M, c.ref[k]) < TOL, (name, k)
    A, b = d.assemble_matrix_rhs(g, data)
    assert rel_max_err(A, c.ref["A"]) < TOL
    assert np.linalg.norm(b - c.ref_rhs) <= TOL * np.linalg.norm(c.ref_rhs)
    # lazily fetched matrices of a tilted grid: only the two vector-source matrices carry the lift into the ambient
    # space (applied when they are fetched, their shape known before); the others are plain device-resident proxies
    from porepy_amd.lazy import LazyCsr

    lazy = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": _RawBC(c.bc), "bc_values": c.bc_values,
                                           "ambient_dimension": c.vdim, "vector_source": c.vector_source_values})
    dl = pa.Mpfa("flow", library=lib, lazy=True)
    dl.discretize(g, lazy)
    ml = lazy[pa.DISCRETIZATION_MATRICES]["flow"]
    for k in ALL_KEYS:
        assert isinstance(ml[k], LazyCsr) and not ml[k].materialized, (name, k)
        assert ml[k].shape == c.ref[k].shape, (name, k)
    x = np.linspace(0.0, 1.0, g.num_cells)
    assert np.allclose(ml["flux"] @ x, c.ref["flux"] @ x, rtol=0, atol=TOL * abs(c.ref["flux"]).max())
    assert not ml["flux"].materialized  # (the product ran on the device)
    # a device-side consumer gets the lifted matrix without a fetch: same bits as the host-side lift
    dvs = pa.DeviceCsr.from_any(ml["vector_source"], dl.context(g))
    assert not ml["vector_source"].materialized
    hv = ml["vector_source"].tocsr()
    dv = dvs.to_scipy()
    assert np.array_equal(dv.indptr, hv.indptr) and np.array_equal(dv.indices, hv.indices) and np.array_equal(dv.data, hv.data)
    for k in ALL_KEYS:
        assert rel_max_err(ml[k].tocsr(), c.ref[k]) < TOL, (name, k)
    Al, bl = dl.assemble_matrix_rhs(g, lazy)
    assert rel_max_err(Al, c.ref["A"]) < TOL and np.linalg.norm(bl - c.ref_rhs) <= TOL * np.linalg.norm(c.ref_rhs)


def check_tpfa_case(lib, name: str):
    """Tpfa (and Mpfa on 1-D grids, which delegates to it) against the reference: stored patterns
    bit-exact, values, A and b (numerics/fv/tpfa.py:84-279, mpfa.py:690-712)."""
    c = TiltedCase(name)  # same fixture layout
    g = pa.grid_from_raw(c.grid)
    K = type("K", (), {"values": c.perm})()
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": _RawBC(c.bc), "bc_values": c.bc_values,
                                           "ambient_dimension": c.vdim, "vector_source": c.vector_source_values})
    d = (pa.Mpfa if c.via_mpfa else pa.Tpfa)("flow", library=lib)
    d.discretize(g, data)
    for k in ALL_KEYS:
        M = data[pa.DISCRETIZATION_MATRICES]["flow"][k]
        R = c.ref[k]
        assert M.shape == R.shape, (name, k)
        assert np.array_equal(M.indptr, R.indptr) and np.array_equal(M.indices, R.indices), (name, k)
        assert rel_max_err(M, R) < TOL, (name, k)
    A, b = d.assemble_matrix_rhs(g, data)
    assert rel_max_err(A, c.ref["A"]) < TOL
    assert np.linalg.norm(b - c.ref_rhs) <= TOL * np.linalg.norm(c.ref_rhs)
    src = np.ones(g.num_cells)
    x, info = d.solve(g, data, source=src, method="bicgstab", rtol=1e-13)
    xo = spla.spsolve(c.ref["A"].tocsc(), c.ref_rhs + src)
    assert np.linalg.norm(x - xo) <= TOL * np.linalg.norm(xo)


def check_zero_dimensional_grid(lib):
    """0-D grids: empty matrices of the right shapes (mpfa.py:129-149)."""
    g = type("Point", (), {"dim": 0, "num_cells": 1, "num_faces": 0, "num_nodes": 1})()
    for cls in (pa.Mpfa, pa.Tpfa):
        data = pa.initialize_data({}, "flow", {"ambient_dimension": 3})
        cls("flow", library=lib).discretize(g, data)
        m = data[pa.DISCRETIZATION_MATRICES]["flow"]
        assert m["flux"].shape == (0, 1) and m["bound_flux"].shape == (0, 0)
        assert m["vector_source"].shape == (0, 3) and m["bound_pressure_vector_source"].shape == (0, 3)


def partial_one_cell_at_a_time(lib):
    """Gradual build: discretize the nodes of one cell at a time and sum the pieces
    (tests/numerics/fv/test_mpfa.py:574-640)."""
    import scipy.sparse as sps

    g = pa.CartGrid([3, 3])
    g.compute_geometry()
    rng = np.random.default_rng(42)
    kxx, kyy = rng.random(g.num_cells) + 0.1, rng.random(g.num_cells) + 0.1
    K = pa.SecondOrderTensor(kxx=kxx, kyy=kyy, kxy=0.5 * rng.random(g.num_cells) * np.sqrt(kxx * kyy))
    bc = pa.BoundaryCondition(g)
    keys = ("flux", "bound_flux", "vector_source")
    acc = {k: None for k in keys}
    covered = np.zeros(g.num_faces, bool)
    discr = pa.Mpfa("flow", library=lib)
    fn, cn = pa.partial._incidence(g)
    for cell in range(g.num_cells):
        nodes = cn[:, cell].nonzero()[0]
        data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "specified_nodes": nodes})
        discr.discretize(g, data)
        af = data[pa.PARAMETERS]["flow"]["active_faces"]
        for k in keys:
            M = data[pa.DISCRETIZATION_MATRICES]["flow"][k].tolil()
            M[np.flatnonzero(covered)] = 0
            acc[k] = M.tocsr() if acc[k] is None else acc[k] + M.tocsr()
        covered[af] = True
    assert covered.all()
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc})
    pa.Mpfa("flow", library=lib).discretize(g, data)
    for k in keys:
        assert rel_max_err(acc[k], data[pa.DISCRETIZATION_MATRICES]["flow"][k]) < TOL, k


def gmres_matches_direct(lib, g, restart=0, seed=1):
    """Jacobi-GMRES(m) on the (non-symmetric) MPFA system against a direct solve of the same system;
    a warm start from the solution must return immediately."""
    rng = np.random.default_rng(seed)
    nc = g.num_cells
    K = pa.SecondOrderTensor(kxx=1 + rng.random(nc), kyy=3 + rng.random(nc), kxy=0.5 * rng.random(nc),
                             **({"kzz": 0.4 + rng.random(nc), "kyz": 0.2 * rng.random(nc)} if g.dim == 3 else {}))
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, list(np.array(["dir", "neu", "dir", "rob"])[np.arange(bf.size) % 4]))
    bv = np.zeros(g.num_faces)
    bv[bf] = rng.random(bf.size)
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "bc_values": bv})
    d = pa.Mpfa("flow", library=lib)
    d.discretize(g, data)
    A, b = d.assemble_matrix_rhs(g, data)
    src = rng.random(nc) * g.cell_volumes
    xo = spla.spsolve(A.tocsc(), b + src)
    x, info = d.solve(g, data, source=src, method="gmres", rtol=1e-13, restart=restart, maxit=5000)
    assert info["converged"] and info["iterations"] > 1
    assert np.linalg.norm(b + src - A @ x) <= 1e-12 * np.linalg.norm(b + src)
    assert np.linalg.norm(x - xo) <= TOL * np.linalg.norm(xo)
    xb, ib = d.solve(g, data, source=src, method="bicgstab", rtol=1e-13)
    assert np.linalg.norm(x - xb) <= TOL * np.linalg.norm(xo)
    x2, info2 = d.solve(g, data, source=src, method="gmres", rtol=1e-9, x0=x)
    assert info2["iterations"] == 0 and info2["converged"]
    return info


def linear_field_exact(lib, g, tol=1e-11):
    """Homogeneous anisotropic K, Dirichlet p = a.x: MPFA reproduces it exactly."""
    nc = g.num_cells
    K = pa.SecondOrderTensor(kxx=np.ones(nc), kyy=3 * np.ones(nc), kzz=0.3 * np.ones(nc),
                             kxy=0.4 * np.ones(nc), kxz=0.05 * np.ones(nc) if g.dim == 3 else None,
                             kyz=0.1 * np.ones(nc) if g.dim == 3 else None)
    a = np.array([1.0, -2.0, 0.5])
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    bv = np.zeros(g.num_faces)
    bv[bf] = a[: g.dim] @ g.face_centers[: g.dim, bf]
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "bc_values": bv})
    d = pa.Mpfa("flow", library=lib)
    d.discretize(g, data)
    x, info = d.solve(g, data, rtol=1e-13)
    exact = a[: g.dim] @ g.cell_centers[: g.dim]
    assert info["converged"]
    assert np.max(np.abs(x - exact)) < tol * max(1.0, np.max(np.abs(exact))), np.max(np.abs(x - exact))
    # constant pressure -> zero flux on every face: (flux + bound_flux restricted) rows sum to 0
    mats = data[pa.DISCRETIZATION_MATRICES]["flow"]
    ones_c = np.ones(nc)
    ones_f = np.zeros(g.num_faces)
    ones_f[bf] = 1.0
    q = mats["flux"] @ ones_c + mats["bound_flux"] @ ones_f
    assert np.max(np.abs(q)) < 1e-10 * abs(mats["flux"]).max()
    return info


# ------------------------------------------------------------------------------------ MPSA
from oracle import mpsa_oracle as so  # noqa: E402
from tests._golden import MPSA_KEYS, MpsaCase  # noqa: E402

MPSA_WHICH = dict(zip(MPSA_KEYS, (7, 8, 9, 10)))


def run_mpsa_case(lib, c: MpsaCase):
    ctx = pa.Context(0, lib)
    ctx.set_grid(c.grid)
    eta = c.eta if c.eta is not None else mo.default_eta(c.grid["name"])
    ctx.mpsa_set_params(c.stiffness, c.grid["cell_volumes"], c.bc["is_dir"], c.bc["is_neu"], eta,
                        is_rob=c.bc.get("is_rob"), robin_weight=c.bc.get("robin_weight"), basis=c.bc.get("basis"))
    if getattr(c, "eta_sub", None) is not None:
        ctx.mpsa_set_subface_eta(c.eta_sub)
    if getattr(c, "hf_eta", None) is not None:
        ctx.mpsa_set_reconstruction_eta(c.hf_eta)
    ctx.mpsa_discretize()
    return ctx


def check_mpsa_golden_case(lib, name: str):
    c = MpsaCase(name)
    TOL = tol_for(name)  # noqa: N806
    ctx = run_mpsa_case(lib, c)
    ora = so.discretize(c.grid, c.stiffness, c.bc, eta=c.eta_sub if c.eta_sub is not None else c.eta, hf_eta=c.hf_eta)
    for k in MPSA_KEYS:
        M = ctx.matrix(MPSA_WHICH[k])
        assert M.indices.dtype == np.int32 and M.has_sorted_indices
        assert np.array_equal(M.indptr, ora[k].indptr), (name, k)
        assert np.array_equal(M.indices, ora[k].indices), (name, k)
        assert rel_max_err(M, ora[k]) < TOL, (name, k)
        if k in c.ref:
            assert rel_max_err(M, c.ref[k]) < TOL, (name, k)
            subset, outside, _ = check_pattern(M, c.ref[k])
            assert subset and outside < 1e-12, (name, k, outside)
    ctx.mpsa_assemble(c.bc_values, c.source)
    A = ctx.matrix(pa._lib.MAT_MECH_SYSTEM)
    n = A.shape[0]
    b = ctx.active_rhs(n)
    assert rel_max_err(A, c.ref["A"]) < TOL
    assert np.linalg.norm(b - c.ref_rhs) <= TOL * max(np.linalg.norm(c.ref_rhs), 1e-300)
    x, info = ctx.solve("bicgstab", rtol=1e-13, maxit=20000, n=n)
    assert info["converged"]
    res = np.linalg.norm(c.ref_rhs - c.ref["A"] @ x) / max(np.linalg.norm(c.ref_rhs), 1e-300)
    assert res < (1e-8 if "sliver" in name else 1e-10), (name, res)
    if "hetero" not in name and "sliver" not in name:
        assert np.linalg.norm(x - c.ref_x) <= 1e-8 * np.linalg.norm(c.ref_x), name
    ctx.close()


def check_mpsa_subface_case(lib, name: str, scramble: bool = False):
    """Conditions per sub-face (mpsa.py:712-720, 752-754, 780-781, 1127-1138): through the C ABI against the
    oracle (exact pattern) and the matrices the reference produced; through the host mirror with the
    caller's face_nodes stored unsorted (``scramble``: the sub-face numbering then differs from the device's)."""
    from tests._golden import MpsaSubfaceCase

    c = MpsaSubfaceCase(name)
    nd = c.grid["dim"]
    ora = so.discretize(c.grid, c.stiffness, c.bc, hf_eta=c.hf_eta)
    if not scramble:
        ctx = pa.Context(0, lib)
        ctx.set_grid(c.grid)
        nf = c.grid["face_centers"].shape[1]
        ctx.mpsa_set_params(c.stiffness, c.grid["cell_volumes"], np.zeros((nd, nf), bool), np.ones((nd, nf), bool),
                            mo.default_eta(c.grid["name"]))
        ctx.mpsa_set_subface_bc(c.bc["is_dir"], c.bc["is_neu"], c.bc["is_rob"], c.bc["robin_weight"],
                                basis_sub=c.bc.get("basis"))
        if c.hf_eta is not None:
            ctx.mpsa_set_reconstruction_eta(c.hf_eta)
        ctx.mpsa_discretize()
        for k in MPSA_KEYS:
            M = ctx.matrix(MPSA_WHICH[k])
            assert M.shape == c.ref[k].shape, (name, k, M.shape)
            assert M.indices.dtype == np.int32 and M.has_sorted_indices
            assert np.array_equal(M.indptr, ora[k].indptr), (name, k)
            assert np.array_equal(M.indices, ora[k].indices), (name, k)
            assert rel_max_err(M, ora[k]) < TOL, (name, k)
            assert rel_max_err(M, c.ref[k]) < TOL, (name, k)
        with pytest.raises(pa._lib.PorefvError, match="sub-face rows"):
            ctx.mpsa_assemble(np.zeros(nd * nf), None)
        # back to conditions per face on the same handle
        ctx.mpsa_set_params(c.stiffness, c.grid["cell_volumes"], np.ones((nd, nf), bool), np.zeros((nd, nf), bool),
                            mo.default_eta(c.grid["name"]))
        ctx.mpsa_discretize()
        assert ctx.matrix(MPSA_WHICH["stress"]).shape == (nd * nf, nd * c.grid["cell_centers"].shape[1])
        ctx.close()
        return
    # host mirror, unsorted storage of face_nodes
    import scipy.sparse as sps

    g = pa.grid_from_raw(c.grid)
    fn = sps.csc_matrix(g.face_nodes)
    rng = np.random.default_rng(11)
    ind, dat = fn.indices.copy(), fn.data.copy()
    perm = np.arange(ind.size)
    for f in range(fn.shape[1]):
        a, b = fn.indptr[f], fn.indptr[f + 1]
        perm[a:b] = a + rng.permutation(b - a)
    g.face_nodes = sps.csc_matrix((dat[perm], ind[perm], fn.indptr), shape=fn.shape)
    # conditions in the caller's (scrambled) sub-face order; perm[p_caller] = sorted position
    bc = pa.BoundaryConditionVectorial(g)
    bc.is_dir, bc.is_neu, bc.is_rob = c.bc["is_dir"][:, perm], c.bc["is_neu"][:, perm], c.bc["is_rob"][:, perm]
    bc.robin_weight = c.bc["robin_weight"][:, :, perm]
    bc.basis = (np.tile(np.eye(nd)[:, :, None], (1, 1, perm.size)) if c.bc.get("basis") is None
                else c.bc["basis"][:, :, perm])
    bc.num_faces = perm.size
    C = pa.FourthOrderTensor.from_values(c.stiffness) if hasattr(pa.FourthOrderTensor, "from_values") else None
    if C is None:
        C = pa.FourthOrderTensor(np.ones(g.num_cells), np.ones(g.num_cells))
        C.values = c.stiffness
    par = {"fourth_order_tensor": C, "bc": bc}
    if c.hf_eta is not None:
        par["reconstruction_eta"] = c.hf_eta
    data = pa.initialize_data({}, "mechanics", par)
    pa.Mpsa("mechanics", library=lib).discretize(g, data)
    md = data[pa.DISCRETIZATION_MATRICES]["mechanics"]
    blk = (nd * perm[:, None] + np.arange(nd)[None, :]).ravel()  # caller block -> sorted block
    for k in MPSA_KEYS:
        ref = c.ref[k]
        if k in ("stress", "bound_stress"):
            ref = ref[blk]
        if k in ("bound_stress", "bound_displacement_face"):
            ref = ref[:, blk]
        assert md[k].shape == ref.shape
        assert rel_max_err(md[k], ref.tocsr()) < TOL, (name, k)


def check_mpsa_known_answer(lib, key: str):
    """The reference's golden displacement / traction vectors (test_mpsa.py:1296-1323)."""
    c = MpsaCase("mpsa_known_" + key)
    ctx = run_mpsa_case(lib, c)
    ctx.mpsa_assemble(c.bc_values, c.known_rhs)
    n = c.grid["dim"] * c.grid["cell_centers"].shape[1]
    u, info = ctx.solve("bicgstab", rtol=1e-13, maxit=20000, n=n)
    stress = ctx.spmv(pa._lib.MAT_STRESS, u) + ctx.spmv(pa._lib.MAT_BOUND_STRESS, c.bc_values)
    assert np.allclose(u, c.known_u)
    assert np.allclose(stress, c.known_stress)


def mpsa_uniaxial_exact(lib, g, tol=1e-10, precond="jacobi"):
    """BASELINE config C4 recipe: mu = lambda = 1, rollers on the low x/y/z faces, unit traction on
    top; exact u = (nu x / E, nu y / E, -z / E), E = 2.5, nu = 0.25."""
    nd = g.dim
    nc, nf = g.num_cells, g.num_faces
    C = pa.FourthOrderTensor(np.ones(nc), np.ones(nc))
    bc = pa.BoundaryConditionVectorial(g)
    bf = g.get_all_boundary_faces()
    fc = g.face_centers
    for axis in range(nd):
        roll = bf[fc[axis, bf] < 1e-9]
        bc.is_dir[axis, roll] = True
        bc.is_neu[axis, roll] = False
    bv = np.zeros((nd, nf))
    top = bf[fc[nd - 1, bf] > fc[nd - 1].max() - 1e-9]
    bv[nd - 1, top] = -1.0 * g.face_areas[top]
    data = pa.initialize_data({}, "mechanics", {"fourth_order_tensor": C, "bc": bc, "bc_values": bv.ravel("F")})
    d = pa.Mpsa("mechanics", library=lib)
    d.discretize(g, data)
    u, info = d.solve(g, data, rtol=1e-13, precond=precond)
    assert info["converged"]
    u = u.reshape(nd, -1, order="F")
    cc = g.cell_centers
    if nd == 3:
        E, nu = 2.5, 0.25
        exact = np.vstack((nu * cc[0] / E, nu * cc[1] / E, -cc[2] / E))
    else:  # plane strain: sigma_yy = -1, eps_xx free in x only
        lam = mu = 1.0
        eyy = -1.0 / (lam + 2 * mu - lam * lam / (lam + 2 * mu))
        exx = -lam / (lam + 2 * mu) * eyy
        exact = np.vstack((exx * cc[0], eyy * cc[1]))
    assert np.max(np.abs(u - exact)) < tol, np.max(np.abs(u - exact))
    return info


def mpsa_operator_roundtrip(lib, g, seed=0, mode="clamped_bottom"):
    """Mpsa operator API on one of this package's grids vs the oracle (heterogeneous Lame
    parameters, bottom clamped or rollers on the low-x side, Neumann elsewhere)."""
    rng = np.random.default_rng(seed)
    nd, nc, nf = g.dim, g.num_cells, g.num_faces
    het = np.where(g.cell_centers[0] > 0.5 * g.nodes[0].max(), 50.0, 1.0)
    C = pa.FourthOrderTensor(het * (1 + rng.random(nc)), het * (1 + rng.random(nc)))
    bc = pa.BoundaryConditionVectorial(g)
    bf = g.get_all_boundary_faces()
    bot = bf[g.face_centers[nd - 1, bf] < 1e-9]
    bc.is_dir[:, bot] = True
    bc.is_neu[:, bot] = False
    if mode == "roller":
        west = bf[g.face_centers[0, bf] < 1e-9]
        bc.is_dir[0, west] = True
        bc.is_neu[0, west] = False
        bc.is_dir[1:, west] = False
        bc.is_neu[1:, west] = True
    bv = (rng.random((nd, nf)) - 0.4) * (bc.is_dir | bc.is_neu)
    src = 0.1 * rng.random(nd * nc)
    data = pa.initialize_data({}, "mechanics", {"fourth_order_tensor": C, "bc": bc,
                                                "bc_values": bv.ravel("F"), "source": src})
    d = pa.Mpsa("mechanics", library=lib)
    d.discretize(g, data)
    raw = pa.grid_to_raw(g)
    ora = so.discretize(raw, C.values, {"is_dir": bc.is_dir, "is_neu": bc.is_neu})
    mats = data[pa.DISCRETIZATION_MATRICES]["mechanics"]
    for k in MPSA_KEYS:
        assert np.array_equal(mats[k].indices, ora[k].indices), k
        assert rel_max_err(mats[k], ora[k]) < TOL, k
    A, b = d.assemble_matrix_rhs(g, data)
    Ao, bo = so.assemble_matrix_rhs(raw, ora, bv.ravel("F"), src)
    assert rel_max_err(A, Ao) < TOL
    assert np.linalg.norm(b - bo) <= TOL * np.linalg.norm(bo)
    x, info = d.solve(g, data, rtol=1e-13)
    assert info["converged"]
    assert np.linalg.norm(bo - Ao @ x) <= 1e-10 * np.linalg.norm(bo)
    return d, data


def check_mpsa_partial_case(lib, name: str):
    """specified_* and update_discretization for MPSA against the reference (mpsa.py:196-216, 383-487)."""
    c = MpsaPartialCase(name)
    g = pa.grid_from_raw(c.grid)
    nd = g.dim
    bc = pa.BoundaryConditionVectorial(g)
    bc.is_dir, bc.is_neu = c.is_dir.copy(), c.is_neu.copy()
    C = pa.FourthOrderTensor(c.mu, c.lam)
    full = pa.initialize_data({}, "mech", {"fourth_order_tensor": C, "bc": bc})
    d_full = pa.Mpsa("mech", library=lib)
    d_full.discretize(g, full)
    full_m = {k: v.copy() for k, v in full[pa.DISCRETIZATION_MATRICES]["mech"].items()}
    for sub in c.partial:
        data = pa.initialize_data({}, "mech", {"fourth_order_tensor": C, "bc": bc, **sub["spec"]})
        pa.Mpsa("mech", library=lib).discretize(g, data)
        af = sub["active_faces"]
        assert np.array_equal(data[pa.PARAMETERS]["mech"]["active_faces"], af)
        rows = (nd * af[:, None] + np.arange(nd)[None, :]).ravel()
        other = np.setdiff1d(np.arange(nd * g.num_faces), rows)
        for k in MPSA_KEYS:
            M = data[pa.DISCRETIZATION_MATRICES]["mech"][k]
            assert rel_max_err(M, sub["mats"][k]) < TOL, (name, sub["spec"], k)
            assert M[other].nnz == 0
            assert rel_max_err(M[rows], full_m[k][rows]) < TOL
    full[pa.PARAMETERS]["mech"]["fourth_order_tensor"] = pa.FourthOrderTensor(c.mu_new, c.lam_new)
    full["update_discretization"] = {"modified_cells": c.modified_cells}
    d_full.update_discretization(g, full)
    for k in ("stress", "bound_stress"):
        assert rel_max_err(full[pa.DISCRETIZATION_MATRICES]["mech"][k], c.updated[k]) < TOL, (name, "update", k)
    _, touched = pa.active_indices(g, cells=c.modified_cells)
    untouched = np.setdiff1d(np.arange(g.num_faces), touched)
    if untouched.size:
        rows = (nd * untouched[:, None] + np.arange(nd)[None, :]).ravel()
        assert np.array_equal(full[pa.DISCRETIZATION_MATRICES]["mech"]["stress"][rows].data, full_m["stress"][rows].data)


def amg_filter_layout_states(lib, n=6):
    """Strength filter of the AMG setup (amg_filter): the row layout of the previous filtering is offered again only
    after a setup that reproduced it; a try that does not fit costs one repeat and withdraws the offer.  States of
    ``stats()["amg_filter_layout"]``: 0 counted + scanned, 1 wrote into the kept layout, 2 tried, did not fit, redone.
    Every solve is checked against the direct solution."""
    g = pa.StructuredTetrahedralGrid([n, n, n], [1, 1, 1])
    g.compute_geometry()
    rng = np.random.default_rng(2)
    nc = g.num_cells
    bf = g.get_all_boundary_faces()
    xf = g.face_centers[0, bf]
    dirf = bf[(xf < 1e-9) | (xf > 1 - 1e-9)]
    bc = pa.BoundaryCondition(g, dirf, ["dir"] * dirf.size)
    bv = np.zeros(g.num_faces)
    bv[dirf] = g.face_centers[0, dirf]

    def tensor(sc):
        return pa.SecondOrderTensor(kxx=sc, kyy=5 * sc, kxy=0.4 * sc, kzz=0.2 * sc, kyz=0.1 * sc)

    s1 = np.exp(0.5 * rng.standard_normal(nc))
    s2 = s1 * np.exp(0.1 * rng.standard_normal(nc))
    s3 = s1 * np.exp(1.0 * rng.standard_normal(nc))
    data = pa.initialize_data({}, "flow", {"second_order_tensor": tensor(s1), "bc": bc, "bc_values": bv})
    d = pa.Mpfa("flow", library=lib)
    states = []
    for sc in (s1, s1, s1, s2, s3, s2, s2, s2):
        data[pa.PARAMETERS]["flow"]["second_order_tensor"] = tensor(sc)
        d.discretize(g, data)
        A, b = d.assemble_matrix_rhs(g, data)
        x, info = d.solve(g, data, source=g.cell_volumes, method="bicgstab", rtol=1e-12, precond="amg")
        xo = spla.spsolve(A.tocsc(), b + g.cell_volumes)
        assert info["converged"] and np.linalg.norm(x - xo) <= TOL * np.linalg.norm(xo)
        states.append(int(d.context(g).stats()["amg_filter_layout"]))
    assert states == [0, 0, 1, 2, 0, 0, 0, 1], states
    return states


def amg_fused_cycle_is_the_same_operator(lib, g, env=None, rtol=1e-12):
    """The fused forms of the cycle's larger coarse levels (PFV_AMG_FUSE_CYCLE, amg.inc: amg_cycle -- the prolongation inside
    the post-smoothing product, the second visit's residual + first smoothing step in one product, its correction folded
    into the parent's prolongation) apply the SAME linear operator as the launches they replace: same iteration count, the
    same solution to rounding, fewer launches.  ``env``: extra switches that bring the fused forms into play on a small
    grid (PFV_AMG_FUSE_ROWS=0: no level takes the small-level launches; PFV_AMG_GAMMA=2: first coarse level visited twice)."""
    rng = np.random.default_rng(4)
    nc = g.num_cells
    sc = np.exp(0.5 * rng.standard_normal(nc))
    kw = dict(kxx=sc, kyy=3 * sc, kxy=0.3 * sc)
    if g.dim == 3:
        kw.update(kzz=0.4 * sc, kyz=0.1 * sc)
    bf = g.get_all_boundary_faces()
    xf = g.face_centers[0, bf]
    dirf = bf[(xf < 1e-9) | (xf > g.nodes[0].max() - 1e-9)]
    bv = np.zeros(g.num_faces)
    bv[dirf] = g.face_centers[0, dirf]
    keys = dict(env or {})
    keys.setdefault("PFV_AMG_FUSE_CYCLE", "1")
    saved = {k: os.environ.get(k) for k in keys}
    res = {}
    try:
        for fused in ("0", "1"):
            for k, v in keys.items():
                os.environ[k] = v
            os.environ["PFV_AMG_FUSE_CYCLE"] = fused
            data = pa.initialize_data({}, "flow", {"second_order_tensor": pa.SecondOrderTensor(**kw),
                                                   "bc": pa.BoundaryCondition(g, dirf, ["dir"] * dirf.size), "bc_values": bv})
            d = pa.Mpfa("flow", library=lib)
            d.discretize(g, data)
            d.assemble_matrix_rhs(g, data)
            x, info = d.solve(g, data, source=g.cell_volumes, method="bicgstab", rtol=rtol, precond="amg")
            assert info["converged"], (fused, info)
            st = d.context(g).stats()
            res[fused] = (x, info["iterations"], int(st.get("solve_launches", 0)), int(st["amg_levels"]))
            d.context(g).close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    (x0, it0, l0, lev), (x1, it1, l1, _) = res["0"], res["1"]
    assert lev >= 3, lev  # (a coarse level with a level below it: something to fuse)
    assert abs(it1 - it0) <= 1, (it0, it1)
    assert np.linalg.norm(x1 - x0) <= 1e-9 * np.linalg.norm(x0)
    return {"iterations": (it0, it1), "launches": (l0, l1), "levels": lev}


def amg_preconditioner(lib, g, seed=2, hetero_sigma=0.5):
    """Aggregation-AMG-preconditioned solves against the direct solution of the same system, far fewer
    iterations than Jacobi, bitwise repeatable."""
    rng = np.random.default_rng(seed)
    nc = g.num_cells
    sc = np.exp(hetero_sigma * rng.standard_normal(nc))
    kw = dict(kxx=sc, kyy=5 * sc, kxy=0.4 * sc)
    if g.dim == 3:
        kw.update(kzz=0.2 * sc, kyz=0.1 * sc)
    K = pa.SecondOrderTensor(**kw)
    bf = g.get_all_boundary_faces()
    xf = g.face_centers[0, bf]
    dirf = bf[(xf < 1e-9) | (xf > g.nodes[0].max() - 1e-9)]
    bc = pa.BoundaryCondition(g, dirf, ["dir"] * dirf.size)
    bv = np.zeros(g.num_faces)
    bv[dirf] = g.face_centers[0, dirf]
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "bc_values": bv})
    d = pa.Mpfa("flow", library=lib)
    d.discretize(g, data)
    A, b = d.assemble_matrix_rhs(g, data)
    src = g.cell_volumes
    xo = spla.spsolve(A.tocsc(), b + src)
    xj, ij = d.solve(g, data, source=src, rtol=1e-12)
    out = {}
    for method in ("bicgstab", "gmres"):
        x, info = d.solve(g, data, source=src, method=method, rtol=1e-12, precond="amg")
        assert info["converged"], method
        assert np.linalg.norm(x - xo) <= TOL * np.linalg.norm(xo), method
        out[method] = info["iterations"]
    assert out["bicgstab"] * 4 < ij["iterations"], (out, ij["iterations"])
    x2, info2 = d.solve(g, data, source=src, method="bicgstab", rtol=1e-12, precond="amg")
    x3, info3 = d.solve(g, data, source=src, method="bicgstab", rtol=1e-12, precond="amg")
    assert np.array_equal(x2, x3) and info2["iterations"] == info3["iterations"]
    st = d.context(g).stats()
    # (entries of all the cycle's matrices over nnz(A): below 1 when the strength filter thins the finest level too)
    assert st["amg_levels"] >= 2 and 0.2 < st["amg_operator_complexity"] < 2.0
    assert st["amg_maps_reused"] == 0  # first hierarchy of this pattern
    assert st["amg_filter_layout"] == 0  # (one setup so far -- the repeated solves reuse the hierarchy as it is)
    # new parameter values on the same grid: the patterns stay, the hierarchy keeps its aggregates and
    # redoes the Galerkin products only; the solve is still right and about as fast
    sc2 = sc * np.exp(0.1 * rng.standard_normal(nc))
    kw2 = {k: v * sc2 / sc for k, v in kw.items()}
    data[pa.PARAMETERS]["flow"]["second_order_tensor"] = pa.SecondOrderTensor(**kw2)
    d.discretize(g, data)
    A2, b2 = d.assemble_matrix_rhs(g, data)
    xo2 = spla.spsolve(A2.tocsc(), b2 + src)
    xr, ir = d.solve(g, data, source=src, method="bicgstab", rtol=1e-12, precond="amg")
    st2 = d.context(g).stats()
    assert st2["amg_maps_reused"] == 1
    assert ir["converged"] and np.linalg.norm(xr - xo2) <= TOL * np.linalg.norm(xo2)
    assert ir["iterations"] <= out["bicgstab"] + 4, (ir["iterations"], out)
    # a rebuilt discretization (new sub-cell topology, new symbolic phase) reuses exactly when its pattern is proved
    # equal to the saved one -- sizes and the checksum of A's index arrays the symbolic phase leaves; with
    # PFV_AMG_REUSE_REBUILT=0 the symbolic phase itself has to be the same one
    data[pa.PARAMETERS]["flow"]["hip_rebuild_topology"] = True
    d.discretize(g, data)
    d.assemble_matrix_rhs(g, data)
    xf, i_f = d.solve(g, data, source=src, method="bicgstab", rtol=1e-12, precond="amg")
    assert d.context(g).stats()["amg_maps_reused"] == 1
    assert np.array_equal(xf, xr) and i_f["iterations"] == ir["iterations"]  # same aggregates, same values: same bits
    # (round 6: a rebuilt topology that is proved unchanged keeps the symbolic phase's outputs -- the SAME symbolic phase,
    # so the maps survive even with PFV_AMG_REUSE_REBUILT=0 ...)
    os.environ["PFV_AMG_REUSE_REBUILT"] = "0"
    try:
        d.discretize(g, data)
        assert d.context(g).stats()["symbolic_reused"] == 1
        d.assemble_matrix_rhs(g, data)
        xf, i_f = d.solve(g, data, source=src, method="bicgstab", rtol=1e-12, precond="amg")
        assert d.context(g).stats()["amg_maps_reused"] == 1
        assert np.array_equal(xf, xr)
        # (... and only a symbolic phase that really ran again, PFV_SYMB_REUSE=0, makes them a different epoch's)
        os.environ["PFV_SYMB_REUSE"] = "0"
        try:
            d.discretize(g, data)
        finally:
            del os.environ["PFV_SYMB_REUSE"]
        assert d.context(g).stats()["symbolic_reused"] == 0
        d.assemble_matrix_rhs(g, data)
        xf, i_f = d.solve(g, data, source=src, method="bicgstab", rtol=1e-12, precond="amg")
        assert d.context(g).stats()["amg_maps_reused"] == 0
    finally:
        del os.environ["PFV_AMG_REUSE_REBUILT"]
    assert np.linalg.norm(xf - xo2) <= TOL * np.linalg.norm(xo2)
    return out, ij["iterations"], st


def check_biot_case(lib, name: str):
    """Biot operator class: MPSA matrices + the five coupling terms per coupling tensor against the
    oracle (exact pattern) and against what the reference's pp.Biot produced."""
    c = BiotCase(name)
    g = pa.grid_from_raw(c.grid)
    bc = pa.BoundaryConditionVectorial(g)
    bc.is_dir, bc.is_neu, bc.is_rob = c.bc["is_dir"].copy(), c.bc["is_neu"].copy(), c.bc["is_rob"].copy()
    bc.robin_weight = c.bc["robin_weight"]
    C = type("C", (), {"values": c.stiffness})()
    maps = {k: type("A", (), {"values": v})() for k, v in c.alphas.items()}
    more = {} if c.eta_sub is None else {"mpsa_eta": c.eta_sub}  # (round 5: continuity points per sub-face)
    data = pa.initialize_data({}, "mechanics", {"fourth_order_tensor": C, "bc": bc, "scalar_vector_mappings": maps, **more})
    d = pa.Biot("mechanics", library=lib)
    d.discretize(g, data)
    md = data[pa.DISCRETIZATION_MATRICES]["mechanics"]
    ora = so.discretize(c.grid, c.stiffness, c.bc, alphas=c.alphas, eta=c.eta_sub)
    for k in ("stress", "bound_stress"):
        assert rel_max_err(md[k], c.ref_mech[k]) < TOL, (name, k)
    for k in BIOT_KEYS:
        for key in c.alphas:
            M = md[k][key]
            assert M.shape == c.ref[k][key].shape, (name, k, key)
            assert M.indices.dtype == np.int32 and M.has_sorted_indices
            assert np.array_equal(M.indptr, ora[k][key].indptr) and np.array_equal(M.indices, ora[k][key].indices), (name, k, key)
            assert rel_max_err(M, ora[k][key]) < TOL, (name, k, key)
            assert rel_max_err(M, c.ref[k][key]) < TOL, (name, k, key)
    # ``reconstruction_eta`` is never read by the reference's Biot (biot.py:803-805 reconstructs at eta): the same matrices
    data2 = pa.initialize_data({}, "mechanics", {"fourth_order_tensor": C, "bc": bc, "scalar_vector_mappings": maps,
                                                "reconstruction_eta": 0.05, **more})
    pa.Biot("mechanics", library=lib).discretize(g, data2)
    md2 = data2[pa.DISCRETIZATION_MATRICES]["mechanics"]
    for k in ("bound_displacement_cell", "bound_displacement_face"):
        assert abs(md2[k] - md[k]).max() == 0.0, (name, k)
    for key in c.alphas:
        assert abs(md2["bound_displacement_pressure"][key] - md["bound_displacement_pressure"][key]).max() == 0.0


def check_subface_case(lib, name: str, scramble: bool = False):
    """Boundary conditions per sub-face (mpfa.py:761-768): flux / bound_flux / the trace matrices with
    sub-face rows against the reference and the oracle.  scramble = True stores face_nodes with the
    node order inside every column reversed: sub-face data and results then follow that numbering."""
    import scipy.sparse as sps

    c = SubfaceCase(name)
    g = pa.grid_from_raw(c.grid)
    nsub = c.grid["fn_indices"].size
    perm = np.arange(nsub)
    if scramble:
        fn = g.face_nodes.tocsc()
        ptr = fn.indptr
        perm = np.concatenate([np.arange(ptr[f], ptr[f + 1])[::-1] for f in range(g.num_faces)])  # user pos -> sorted pos
        g.face_nodes = sps.csc_matrix((fn.data[perm], fn.indices[perm], ptr.copy()), shape=fn.shape)
        assert not g.face_nodes.has_sorted_indices or g.dim == 1
    bc = _RawBC({k: (np.asarray(v)[perm] if np.asarray(v).size == nsub else v) for k, v in c.bc.items()})
    K = type("K", (), {"values": c.perm})()
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc})
    d = pa.Mpfa("flow", library=lib)
    d.discretize(g, data)
    ora = mo.discretize(c.grid, c.perm, c.bc)
    inv = np.argsort(perm)  # sorted pos -> user pos
    for k in ALL_KEYS:
        M = data[pa.DISCRETIZATION_MATRICES]["flow"][k]
        ref = c.ref[k]
        if scramble and "vector_source" not in k:  # bring the reference to the scrambled numbering
            coo = ref.tocoo()
            cols = inv[coo.col] if k in ("bound_flux", "bound_pressure_face") else coo.col
            ref = sps.csr_matrix((coo.data, (inv[coo.row], cols)), shape=ref.shape)
        assert M.shape == ref.shape, (name, k)
        assert rel_max_err(M, ref) < TOL, (name, k, scramble)
        if not scramble:
            assert rel_max_err(M, ora[k]) < TOL, (name, k)
    with pytest.raises(pa.PorefvError):  # flux has sub-face rows: no assembly
        d.assemble_matrix_rhs(g, {**data, pa.PARAMETERS: {"flow": {**data[pa.PARAMETERS]["flow"], "bc_values": np.zeros(g.num_faces)}}})


def device_resident_vectors(lib, g, to_device=None, from_device=None):
    """pfv_set_vectors_on_device: bc values / source / solution exchanged as device buffers give the
    same system and solution as the host-array calls.  ``to_device(array) -> (address, keepalive)``;
    the host emulation passes numpy addresses."""
    rng = np.random.default_rng(4)
    nc, nf = g.num_cells, g.num_faces
    K = pa.SecondOrderTensor(kxx=1 + rng.random(nc), kyy=2 + rng.random(nc), kzz=(0.5 + rng.random(nc)) if g.dim == 3 else None)
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    bv = np.zeros(nf)
    bv[bf] = rng.random(bf.size)
    src = rng.random(nc) * g.cell_volumes
    ctx = pa.Context(0, lib)
    ctx.set_grid(pa.grid_to_raw(g))
    ctx.set_params(K.values, pa.bc_flags(bc), bc.robin_weight, pa.determine_eta(g))
    ctx.discretize()
    ctx.assemble(bv, None, src)
    b_host = ctx.rhs()
    x_host, info_h = ctx.solve("bicgstab", rtol=1e-12, precond="amg")
    if to_device is None:
        to_device = lambda a: (a.ctypes.data, a)  # noqa: E731
        from_device = lambda keep: keep  # noqa: E731
    p_bv, k1 = to_device(np.ascontiguousarray(bv))
    p_src, k2 = to_device(np.ascontiguousarray(src))
    p_x, k3 = to_device(np.zeros(nc))
    ctx.assemble_device(p_bv, 0, p_src)
    assert np.array_equal(ctx.rhs(), b_host)
    info_d = ctx.solve_device(p_x, "bicgstab", rtol=1e-12, precond="amg")
    ctx.sync()
    x_dev = np.asarray(from_device(k3))
    assert info_d["iterations"] == info_h["iterations"]
    assert np.array_equal(x_dev, x_host)
    # and the host calls still work afterwards
    x2, _ = ctx.solve("bicgstab", rtol=1e-12, precond="amg")
    assert np.array_equal(x2, x_host)


def check_periodic_subface_case(lib, name: str, scramble: bool = False):
    """Conditions per sub-face on a grid WITH periodic faces (round 5; _fvutils.py:91-160 numbers the merged sub-faces,
    mpfa.py:761-768, 900-917, 1117-1147): the six matrices against what the reference's ``_flux_discretization``
    produced (oracle/gen_golden_periodic_subface.py).  scramble = True stores the caller's face_nodes with the node
    order inside every column reversed: conditions and results then follow that numbering of the merged sub-faces."""
    import scipy.sparse as sps

    from tests._golden import SubfaceCase

    c = SubfaceCase(name)
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    pmap = z["periodic_face_map"]
    g = pa.grid_from_raw(c.grid)
    g.set_periodic_map(pmap)
    fn = g.face_nodes.tocsc()
    ptr = fn.indptr
    nnf = np.diff(ptr)
    keep = np.ones(g.num_faces, bool)
    keep[pmap[1]] = False
    nsub_u = int(nnf[keep].sum())
    assert c.bc["is_dir"].size == nsub_u
    perm_u = np.arange(nsub_u)  # caller's merged number -> the fixture's merged number
    if scramble:
        perm = np.concatenate([np.arange(ptr[f], ptr[f + 1])[::-1] for f in range(g.num_faces)])
        g.face_nodes = sps.csc_matrix((fn.data[perm], fn.indices[perm], ptr.copy()), shape=fn.shape)
        # merged numbers = ranks among the positions of the kept faces, in storage order
        off = np.concatenate([[0], np.cumsum(np.where(keep, nnf, 0))])
        perm_u = np.concatenate([np.arange(off[f], off[f + 1])[::-1] for f in range(g.num_faces)]).astype(int)
    bc = _RawBC({k: (np.asarray(v)[perm_u] if np.asarray(v).size == nsub_u else v) for k, v in c.bc.items()})
    K = type("K", (), {"values": c.perm})()
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc})
    pa.Mpfa("flow", library=lib).discretize(g, data)
    inv = np.argsort(perm_u)  # fixture's merged number -> caller's
    for k in ALL_KEYS:
        M = data[pa.DISCRETIZATION_MATRICES]["flow"][k]
        ref = c.ref[k]
        if scramble and "vector_source" not in k:
            coo = ref.tocoo()
            cols = inv[coo.col] if k in ("bound_flux", "bound_pressure_face") else coo.col
            ref = sps.csr_matrix((coo.data, (inv[coo.row], cols)), shape=ref.shape)
        assert M.shape == ref.shape, (name, k, M.shape, ref.shape)
        assert rel_max_err(M, ref) < TOL, (name, k, scramble)


def check_periodic_case(lib, name: str, scheme: str = "mpfa"):
    """Grids with periodic faces (Grid.set_periodic_map): all six matrices, A and b of Mpfa / Tpfa
    against the reference (_fvutils.py:91-137, mpfa.py:900-917, tpfa.py:114-262), and the solve."""
    from tests._golden import PeriodicCase

    c = PeriodicCase(name)
    g = pa.grid_from_raw(c.grid)
    g.set_periodic_map(c.periodic_face_map)
    ref = c.ref if scheme == "mpfa" else c.tpfa
    K = type("K", (), {"values": c.perm})()
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": _RawBC(c.bc), "bc_values": c.bc_values,
                                           "vector_source": c.vector_source_values})
    d = (pa.Mpfa if scheme == "mpfa" else pa.Tpfa)("flow", library=lib)
    d.discretize(g, data)
    # The reference's Tpfa reorders the cells of the periodic faces by face but not their signs
    # (tpfa.py:127-146: ci_left[I_left] without left_sgn[I_left]); when the cell_faces signs of the
    # periodic faces differ among themselves (simplex grids) its periodic rows come out with two
    # entries of the same sign.  There the other rows are compared, and ours are checked to be fluxes.
    L, R = c.periodic_face_map
    sg = np.asarray(g.cell_faces.tocsr()[L].sum(axis=1)).ravel()
    ref_defect = scheme == "tpfa" and np.unique(sg).size > 1
    rows = np.setdiff1d(np.arange(g.num_faces), np.r_[L, R]) if ref_defect else np.arange(g.num_faces)
    for k in ALL_KEYS:
        M = data[pa.DISCRETIZATION_MATRICES]["flow"][k]
        assert M.shape == ref[k].shape, (name, k)
        assert rel_max_err(M.tocsr()[rows], ref[k].tocsr()[rows]) < TOL, (name, k)
    if ref_defect:
        F = data[pa.DISCRETIZATION_MATRICES]["flow"]["flux"].tocsr()
        per = F[np.r_[L, R]]
        assert np.all(np.diff(per.indptr) == 2) and abs(per.sum(axis=1)).max() < 1e-12 * abs(per).max()
        assert abs(F[L] - F[R]).max() == 0
        A, b = d.assemble_matrix_rhs(g, data)
        assert abs(A - A.T).max() < 1e-12 * abs(A).max() and abs(A.sum(axis=1)).min() < 1e-12 * abs(A).max()
        return
    A, b = d.assemble_matrix_rhs(g, data)
    assert rel_max_err(A, ref["A"]) < TOL
    assert np.linalg.norm(b - ref["rhs"]) <= TOL * max(np.linalg.norm(ref["rhs"]), 1e-300)
    if np.any(c.bc["is_dir"]):  # (all-periodic / Neumann: singular system)
        src = np.ones(g.num_cells)
        x, info = d.solve(g, data, source=src, method="bicgstab", rtol=1e-13)
        xo = spla.spsolve(ref["A"].tocsc(), ref["rhs"] + src)
        assert np.linalg.norm(x - xo) <= TOL * np.linalg.norm(xo)


def check_biot_partial_case(lib, name: str):
    """Partial discretization of the Biot terms around the nodes of one cell (the reference's own
    test, tests/numerics/fv/test_biot.py:88-198: rows of the active faces / of the cell equal the full
    discretization, every row outside the active sets is zero), then an update after a parameter
    change against a fresh full discretization."""
    c = BiotCase(name)
    g = pa.grid_from_raw(c.grid)
    nd = g.dim

    def make(stiff, alphas):
        bc = pa.BoundaryConditionVectorial(g)
        bc.is_dir, bc.is_neu, bc.is_rob = c.bc["is_dir"].copy(), c.bc["is_neu"].copy(), c.bc["is_rob"].copy()
        bc.robin_weight = c.bc["robin_weight"]
        C = type("C", (), {"values": stiff})()
        maps = {k: type("A", (), {"values": v})() for k, v in alphas.items()}
        return pa.initialize_data({}, "mechanics", {"fourth_order_tensor": C, "bc": bc, "scalar_vector_mappings": maps})

    cn = g.cell_nodes().tocsc()
    face_keys = ("scalar_gradient", "bound_displacement_pressure")
    cell_keys = ("displacement_divergence", "boundary_displacement_divergence", "mpsa_consistency")
    for cell in (0, g.num_cells // 2, g.num_cells - 1):
        data = make(c.stiffness, c.alphas)
        data[pa.PARAMETERS]["mechanics"]["specified_nodes"] = cn.indices[cn.indptr[cell]: cn.indptr[cell + 1]]
        d = pa.Biot("mechanics", library=lib)
        d.discretize(g, data)
        md = data[pa.DISCRETIZATION_MATRICES]["mechanics"]
        af = data[pa.PARAMETERS]["mechanics"]["active_faces"]
        ac = data[pa.PARAMETERS]["mechanics"]["active_cells"]
        assert cell in ac
        rows_f = (nd * af[:, None] + np.arange(nd)[None, :]).ravel()
        off_f = np.setdiff1d(np.arange(nd * g.num_faces), rows_f)
        off_c = np.setdiff1d(np.arange(g.num_cells), ac)
        for k in ("stress", "bound_stress"):
            assert rel_max_err(md[k][rows_f], c.ref_mech[k][rows_f]) < TOL, (name, k)
            assert abs(md[k][off_f]).max() == 0
        for key in c.alphas:
            for k in face_keys:
                assert rel_max_err(md[k][key][rows_f], c.ref[k][key][rows_f]) < TOL, (name, k, key, cell)
                assert abs(md[k][key][off_f]).max() == 0
            for k in cell_keys:
                assert rel_max_err(md[k][key][[cell]], c.ref[k][key][[cell]]) < TOL, (name, k, key, cell)
                if off_c.size:
                    assert abs(md[k][key][off_c]).max() == 0
    # update: new parameters in one cell, rediscretize around it, compare with a full discretization
    rng = np.random.default_rng(5)
    data = make(c.stiffness, c.alphas)
    d = pa.Biot("mechanics", library=lib)
    d.discretize(g, data)
    cell = g.num_cells // 3
    stiff2 = c.stiffness.copy()
    stiff2[..., cell] *= 1.7
    alphas2 = {k: v.copy() for k, v in c.alphas.items()}
    for v in alphas2.values():
        v[..., cell] *= 0.6
    pd = data[pa.PARAMETERS]["mechanics"]
    pd["fourth_order_tensor"] = type("C", (), {"values": stiff2})()
    pd["scalar_vector_mappings"] = {k: type("A", (), {"values": v})() for k, v in alphas2.items()}
    data["update_discretization"] = {"modified_cells": np.array([cell])}
    d.update_discretization(g, data)
    md = data[pa.DISCRETIZATION_MATRICES]["mechanics"]
    full = make(stiff2, alphas2)
    pa.Biot("mechanics", library=lib).discretize(g, full)
    mf = full[pa.DISCRETIZATION_MATRICES]["mechanics"]
    for k in ("stress", "bound_stress", "bound_displacement_cell", "bound_displacement_face"):
        assert rel_max_err(md[k], mf[k]) < 1e-12, (name, k)
    for k in face_keys + cell_keys:
        for key in c.alphas:
            assert rel_max_err(md[k][key], mf[k][key]) < 1e-12, (name, k, key)
    assert rng is not None


def full_size_patch_parity(lib, n_side: int = 69, seeds=(0, None, -1)):
    """Parity at the benchmark's full size (BASELINE configs[2], 1 971 054 tetrahedra) where the oracle
    cannot run on the whole grid: rows of the device matrices of the *full* problem against the oracle
    run on patches cut out of it.  A face row only involves the interaction regions of the face's
    nodes, so on a patch = some cells + one node-ring of halo cells (distributed.extract_subdomain)
    the oracle's rows of the faces of the inner cells are the global rows; the same for the rows of
    A = div flux of the inner cells.  Plus the size-independent checks: the solve's true residual in
    the device system and constant pressure -> zero flux."""
    import bench
    from porepy_amd import distributed as D

    g, K, bc, bv, src = bench.make_problem(n_side)
    raw = pa.grid_to_raw(g)
    nc, nf = g.num_cells, g.num_faces
    flags = pa.bc_flags(bc)
    ctx = pa.Context(0, lib)
    ctx.set_grid(raw)
    ctx.set_params(K.values, flags, bc.robin_weight, pa.determine_eta(g))
    ctx.discretize(skip_vector_source=True)
    ctx.assemble(bv, None, src)
    x, info = ctx.solve("bicgstab", rtol=1e-11, precond="amg")
    assert info["converged"]
    A = ctx.matrix(pa._lib.MAT_SYSTEM)
    b = ctx.rhs()
    assert np.linalg.norm(b - A @ x) <= 1e-10 * np.linalg.norm(b)
    flux = ctx.matrix(pa._lib.MAT_FLUX)
    bflux = ctx.matrix(pa._lib.MAT_BOUND_FLUX)
    ones_f = np.asarray(bc.is_dir, dtype=float)  # p = 1 on the Dirichlet faces, zero Neumann flux
    q = flux @ np.ones(nc) + bflux @ ones_f
    assert np.max(np.abs(q)) < 1e-10 * abs(flux).max()
    cn = g.cell_nodes().tocsc()   # (Nn, Nc)
    nodes_cells = cn.tocsr()
    rng = np.random.default_rng(3)
    raw_bc = pa.params.bc_to_raw(bc)
    checked = 0
    for seed in seeds:
        c0 = {0: 0, -1: nc - 1}.get(seed, int(rng.integers(nc)))
        inner = np.unique(nodes_cells[cn.indices[cn.indptr[c0]: cn.indptr[c0 + 1]]].indices)  # cells around c0
        owner = np.ones(nc, dtype=np.int32)
        owner[inner] = 0
        lp = D.extract_subdomain(raw, owner, 0)
        lbc = {k: np.asarray(raw_bc[k])[lp.face_gid].copy() for k in ("is_dir", "is_neu", "is_rob", "is_internal")}
        lbc["robin_weight"] = np.asarray(raw_bc["robin_weight"], dtype=float)[lp.face_gid]
        art = lp.artificial_boundary
        lbc["is_dir"][art] = False
        lbc["is_rob"][art] = False
        lbc["is_neu"][art] = True
        ora = mo.discretize(lp.raw, np.ascontiguousarray(K.values[:, :, lp.cell_gid]), lbc, eta=pa.determine_eta(g))
        # faces of the inner cells, in local and global numbering
        lcf = lp.raw["cf_indices"][: lp.raw["cf_indptr"][lp.n_own]]
        lfaces = np.unique(lcf)
        gfaces = lp.face_gid[lfaces]
        col_map = np.full(nc, -1)
        col_map[lp.cell_gid] = np.arange(lp.cell_gid.size)
        fmap = np.full(nf, -1)
        fmap[lp.face_gid] = np.arange(lp.face_gid.size)
        for name, M, cmap in (("flux", flux, col_map), ("bound_flux", bflux, fmap)):
            G = M[gfaces].tocoo()
            assert np.all(cmap[G.col] >= 0), name  # the global rows stay inside the patch
            Gl = sps_csr((G.data, (G.row, cmap[G.col])), shape=(gfaces.size, ora[name].shape[1]))
            assert rel_max_err(Gl, ora[name][lfaces]) < TOL, (name, seed)
        Aora, _ = mo.assemble_matrix_rhs(lp.raw, ora, np.zeros(lp.face_gid.size))
        G = A[lp.cell_gid[: lp.n_own]].tocoo()
        assert np.all(col_map[G.col] >= 0)
        Gl = sps_csr((G.data, (G.row, col_map[G.col])), shape=(lp.n_own, lp.cell_gid.size))
        assert rel_max_err(Gl, Aora[: lp.n_own]) < TOL, ("A", seed)
        checked += lfaces.size
    return {"iterations": info["iterations"], "rows_checked": checked}


class PatchCutter:
    """Cuts patches (some cells + one node-ring of halo cells) out of a raw grid, with the incidence
    products of the full grid built once (distributed.extract_subdomain rebuilds them per call)."""

    def __init__(self, raw: dict):
        import scipy.sparse as sps

        self.raw = raw
        nc = raw["cell_centers"].shape[1]
        nf = raw["face_centers"].shape[1]
        nn = raw["nodes"].shape[1]
        self.nc, self.nf, self.nn = nc, nf, nn
        self.cf = sps.csc_matrix((np.ones(raw["cf_indices"].size, dtype=np.int8), raw["cf_indices"], raw["cf_indptr"]),
                                 shape=(nf, nc))
        self.fn = sps.csc_matrix((np.ones(raw["fn_indices"].size, dtype=np.int8), raw["fn_indices"], raw["fn_indptr"]),
                                 shape=(nn, nf))
        self.gsign = sps.csc_matrix((raw["cf_sign"].astype(np.int8), raw["cf_indices"], raw["cf_indptr"]), shape=(nf, nc))
        self.cell_nodes = (self.fn.astype(np.int32) @ self.cf.astype(np.int32)).tocsc()  # nn x nc
        self.node_cells = self.cell_nodes.tocsr()
        self.sides = np.bincount(raw["cf_indices"], minlength=nf)

    def cells_around(self, c0: int) -> np.ndarray:
        cn = self.cell_nodes
        return np.unique(self.node_cells[cn.indices[cn.indptr[c0]: cn.indptr[c0 + 1]]].indices)

    def cut(self, own: np.ndarray):
        import scipy.sparse as sps

        raw = self.raw
        own = np.asarray(own)
        own_nodes = np.unique(self.cell_nodes[:, own].indices)
        ring = np.unique(self.node_cells[own_nodes].indices)
        halo = np.setdiff1d(ring, own)
        cells = np.concatenate([own, halo])
        faces = np.unique(self.cf[:, cells].indices)
        nodes = np.unique(self.fn[:, faces].indices)
        fmap = np.full(self.nf, -1, dtype=np.int64)
        fmap[faces] = np.arange(faces.size)
        nmap = np.full(self.nn, -1, dtype=np.int64)
        nmap[nodes] = np.arange(nodes.size)
        loc_cf = self.gsign[:, cells].tocsc()
        loc_cf = sps.csc_matrix((loc_cf.data, fmap[loc_cf.indices], loc_cf.indptr), shape=(faces.size, cells.size))
        loc_cf.sort_indices()
        loc_fn = self.fn[:, faces].tocsc()
        loc_fn = sps.csc_matrix((loc_fn.data, nmap[loc_fn.indices], loc_fn.indptr), shape=(nodes.size, faces.size))
        loc_fn.sort_indices()
        sides_loc = np.bincount(loc_cf.indices, minlength=faces.size)
        lraw = {
            "dim": raw["dim"], "name": raw.get("name", ""),
            "nodes": np.ascontiguousarray(raw["nodes"][:, nodes]),
            "cf_indptr": loc_cf.indptr.astype(np.int32), "cf_indices": loc_cf.indices.astype(np.int32),
            "cf_sign": loc_cf.data.astype(np.int8),
            "fn_indptr": loc_fn.indptr.astype(np.int32), "fn_indices": loc_fn.indices.astype(np.int32),
            "face_normals": np.ascontiguousarray(raw["face_normals"][:, faces]),
            "face_centers": np.ascontiguousarray(raw["face_centers"][:, faces]),
            "cell_centers": np.ascontiguousarray(raw["cell_centers"][:, cells]),
            "face_areas": np.ascontiguousarray(raw["face_areas"][faces]),
            "cell_volumes": np.ascontiguousarray(raw["cell_volumes"][cells]),
        }
        art = (sides_loc == 1) & (self.sides[faces] == 2)
        return lraw, own.size, cells.astype(np.int64), faces.astype(np.int64), art


def patch_targets(raw: dict, n_random: int = 6, seed: int = 3):
    """Cells to centre patches on: the 8 corners of the bounding box, the centres of its 6 sides (where the
    Dirichlet / Neumann faces and their edges are) and n_random cells anywhere."""
    cc = raw["cell_centers"]
    lo, hi = raw["face_centers"].min(axis=1), raw["face_centers"].max(axis=1)
    pts = []
    for ix in (0, 1):
        for iy in (0, 1):
            for iz in (0, 1):
                pts.append([(lo, hi)[ix][0], (lo, hi)[iy][1], (lo, hi)[iz][2]])
    mid = 0.5 * (lo + hi)
    for d in range(3):
        for side in (lo, hi):
            q = mid.copy()
            q[d] = side[d]
            pts.append(q)
    cells = [int(np.argmin(((cc - np.asarray(q)[:, None]) ** 2).sum(axis=0))) for q in pts]
    rng = np.random.default_rng(seed)
    cells += [int(c) for c in rng.integers(cc.shape[1], size=n_random)]
    return cells


def reference_on_patches(patches, product: bool, keys=None):
    """The REFERENCE ITSELF (pp.Mpfa, python inverter) on patches [(lraw, K, lbc, eta)], in one subprocess
    (tests/_reference_patch_script.py; the live tree in the build container, the byte-compiled archive on the GPU box).
    Returns a list of {key: csr} or None where no reference is importable."""
    import subprocess
    import sys
    import tempfile

    import oracle

    keys = ALL_KEYS if keys is None else keys
    env = oracle.ref_env(prefer_archive=product)
    if env is None:
        return None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory(prefix="pfv_patches_") as d:
        for i, (lraw, K, lbc, eta) in enumerate(patches):
            # (mechanics: the tensor is the (9, 9, Nc) stiffness -- the script then runs pp.Mpsa)
            tensor = {"stiffness": K} if keys is not ALL_KEYS else {"K": K}
            np.savez(os.path.join(d, f"patch_{i:03d}.npz"), is_dir=lbc["is_dir"], is_neu=lbc["is_neu"], eta=eta, **tensor,
                     **{k: v for k, v in lraw.items() if isinstance(v, (np.ndarray, int, str))})
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "_reference_patch_script.py"), d], env=env,
                           cwd="/tmp", capture_output=True, text=True, timeout=1500)
        assert any(l.startswith("RESULT") for l in r.stdout.splitlines()), r.stderr[-2000:]
        out = []
        for i in range(len(patches)):
            z = np.load(os.path.join(d, f"ref_{i:03d}.npz"))
            out.append({k: sps_csr((z[k + "_data"], z[k + "_indices"], z[k + "_indptr"]), shape=tuple(z[k + "_shape"]))
                        for k in keys})
    return out


def grid_patch_parity(lib, raw, Kvals, flags, eta, bv=None, src=None, targets=None, rtol=1e-13, check_solve=True,
                      generic_pattern=False, reference: bool = False):
    """Rows of ALL SIX device matrices and of A = div flux of one full-size problem (raw grid, permeability
    (3,3,Nc), per-face flags 1 = Dirichlet / 2 = Neumann) against the oracle run on patches cut out of it.
    A face row only involves the interaction regions of the face's nodes, so on a patch = some cells + one
    node-ring of halo cells the oracle's rows of the faces of the inner cells are the global rows."""
    nc, nf = raw["cell_centers"].shape[1], raw["face_centers"].shape[1]
    nd = int(raw["dim"])
    ctx = pa.Context(0, lib)
    ctx.set_grid(raw)
    ctx.set_params(Kvals, flags, None, eta)
    ctx.discretize(skip_vector_source=False)
    out = {}
    if bv is not None:
        ctx.assemble(bv, None, src)
    # (rows are fetched patch by patch, pfv_get_matrix_rows: the six matrices of the 2 M-cell grid are 21.6 GB)
    if bv is not None and check_solve:
        x, info = ctx.solve("bicgstab", rtol=rtol, maxit=5000, precond="amg", raise_on_fail=False)
        b = ctx.rhs()
        out["iterations"] = info["iterations"]
        out["true_rel_residual"] = float(np.linalg.norm(b - ctx.spmv(pa._lib.MAT_SYSTEM, x)) / np.linalg.norm(b))
        out["x"] = x
    cutter = PatchCutter(raw)
    is_dir = (flags & 1) != 0
    bc_all = {"is_dir": is_dir, "is_neu": ~is_dir & (cutter.sides == 1), "is_rob": np.zeros(nf, bool),
              "is_internal": np.zeros(nf, bool), "robin_weight": np.ones(nf)}
    targets = patch_targets(raw) if targets is None else targets
    checked, worst = 0, {}
    patterns_checked = 0
    ref_inputs, ref_rows = [], []  # reference = True: the patches and the device rows, compared after the loop
    ex = lambda idx: (nd * np.asarray(idx)[:, None] + np.arange(nd)[None, :]).ravel()  # noqa: E731
    for c0 in targets:
        inner = cutter.cells_around(c0)
        lraw, n_own, cell_gid, face_gid, art = cutter.cut(inner)
        lbc = {k: np.asarray(v)[face_gid].copy() for k, v in bc_all.items()}
        lbc["is_dir"][art] = False
        lbc["is_neu"][art] = True
        ora = mo.discretize(lraw, np.ascontiguousarray(Kvals[:, :, cell_gid]), lbc, eta=eta)
        lfaces = np.unique(lraw["cf_indices"][: lraw["cf_indptr"][n_own]])  # faces of the inner cells
        gfaces = face_gid[lfaces]
        cmap = np.full(nc, -1)
        cmap[cell_gid] = np.arange(cell_gid.size)
        fmap = np.full(nf, -1)
        fmap[face_gid] = np.arange(face_gid.size)
        vmap = np.full(nd * nc, -1)
        vmap[ex(cell_gid)] = np.arange(nd * cell_gid.size)
        if reference:
            ref_inputs.append((lraw, np.ascontiguousarray(Kvals[:, :, cell_gid]), lbc, eta))
            ref_rows.append({"lfaces": lfaces, "interior": cutter.sides[gfaces] == 2})
        for k in ALL_KEYS:
            m = {"flux": cmap, "bound_pressure_cell": cmap, "bound_flux": fmap, "bound_pressure_face": fmap,
                 "vector_source": vmap, "bound_pressure_vector_source": vmap}[k]
            G = ctx.matrix_rows(WHICH[k], gfaces).tocoo()
            assert np.all(m[G.col] >= 0), (k, c0)  # the global rows stay inside the patch
            Gl = sps_csr((G.data, (G.row, m[G.col])), shape=(gfaces.size, ora[k].shape[1]))
            if reference:
                ref_rows[-1][k] = Gl.copy()
            err = rel_max_err(Gl, ora[k][lfaces])
            worst[k] = max(worst.get(k, 0.0), err)
            assert err < TOL, (k, c0, err)
            # sparsity pattern, bit-exact: the rows of the full-size matrix, renumbered into the patch, carry exactly
            # the oracle's column indices (the monotone renumbering keeps them sorted); on a generic grid (perturbed
            # nodes, anisotropic K: the timed one) no stored entry is an exact zero either, i.e. the structural
            # stencil IS the pattern the reference's sparse products leave (north_star: "sparsity pattern bit-exact")
            Ol = sps_csr(ora[k][lfaces])
            Gl.sort_indices()
            Ol.sort_indices()
            assert np.array_equal(Gl.indptr, Ol.indptr) and np.array_equal(Gl.indices, Ol.indices), ("pattern", k, c0)
            patterns_checked += 1
            if generic_pattern:
                # (bound_* columns of boundary faces whose condition does not reach the row are structural zeros in
                # both; only the cell-column matrices are dense in their stencil)
                # rows of Neumann boundary faces are exact zeros in the cell-column matrices (the flux is the datum)
                if k in ("flux", "vector_source"):
                    interior = cutter.sides[gfaces] == 2
                    rows_of = np.repeat(np.arange(gfaces.size), np.diff(Gl.indptr))
                    keep = interior[rows_of]
                    assert np.all(Ol.data[keep] != 0.0) and np.all(Gl.data[keep] != 0.0), ("exact zero in a generic stencil", k, c0)
        if bv is not None:
            Aora, _ = mo.assemble_matrix_rhs(lraw, ora, np.zeros(face_gid.size))
            G = ctx.matrix_rows(pa._lib.MAT_SYSTEM, cell_gid[:n_own]).tocoo()
            assert np.all(cmap[G.col] >= 0)
            Gl = sps_csr((G.data, (G.row, cmap[G.col])), shape=(n_own, cell_gid.size))
            err = rel_max_err(Gl, Aora[:n_own])
            worst["A"] = max(worst.get("A", 0.0), err)
            assert err < TOL, ("A", c0, err)
        checked += lfaces.size
    out.update({"rows_checked": checked, "patches": len(targets), "worst_rel_err": worst,
                "patterns_bit_exact": patterns_checked})
    if reference:
        # ---- the same rows against the REFERENCE ITSELF run on the same patches (same geometry arrays, same tensors)
        is_product = bool(lib.pfv_is_device_build())
        refs = reference_on_patches(ref_inputs, product=is_product)
        out["reference_patches"] = 0 if refs is None else len(refs)
        if refs is not None:
            worst_ref, exact = {}, 0
            for rows, ref in zip(ref_rows, refs):
                for k in ALL_KEYS:
                    Rl = sps_csr(ref[k][rows["lfaces"]])
                    Gl = rows[k]
                    err = rel_max_err(Gl, Rl)
                    worst_ref[k] = max(worst_ref.get(k, 0.0), err)
                    assert err < TOL, ("reference", k, err)
                    # pattern: what the reference stores is stored here (north_star parity metric 1); on the generic
                    # grid the stencils of the cell-column matrices are identical, index for index
                    Rl.sort_indices()
                    Gl.sort_indices()
                    stored = lambda m: sps_csr((np.ones(m.indices.size, np.int8), m.indices, m.indptr), shape=m.shape)  # noqa: E731
                    D = stored(Rl) - stored(Gl)
                    assert D.nnz == 0 or D.max() <= 0, ("the reference stores an entry the device pattern lacks", k)
                    if generic_pattern and k in ("flux", "vector_source"):
                        rows_of = np.repeat(np.arange(Gl.shape[0]), np.diff(Gl.indptr))
                        keep = rows["interior"][rows_of]
                        rows_ref = np.repeat(np.arange(Rl.shape[0]), np.diff(Rl.indptr))
                        keep_ref = rows["interior"][rows_ref]
                        assert np.array_equal(Gl.indices[keep], Rl.indices[keep_ref]), ("pattern vs reference", k)
                        exact += 1
            out["worst_rel_err_vs_reference"] = worst_ref
            out["patterns_bit_exact_vs_reference"] = exact
    return out


def bench_grid_patch_parity(lib, n_side: int = 69, n_random: int = 6):
    """The grid bench.py TIMES (make_slab_problem: hash-perturbed nodes, Morton-numbered cells, log-normal
    full-tensor K, Dirichlet x-faces) at its full size: all six matrices + A on >= 20 patches (box corners,
    side centres, random cells), the true residual of the rtol = 1e-13 solve."""
    import bench

    lp, Kvals, flags, bv, src, eta = bench.make_slab_problem(n_side, 0, 1)
    return grid_patch_parity(lib, lp.raw, Kvals, flags, eta, bv, src, patch_targets(lp.raw, n_random),
                             generic_pattern=True, reference=True)


def config_c2_patch_parity(lib, n_side: int = 32, n_random: int = 6):
    """BASELINE configs[1]: StructuredTetrahedralGrid([32]^3), isotropic K = 1, Dirichlet p = x all round --
    the case where the reference's stored pattern is value dependent (exact zeros on the unperturbed
    lattice); values of all six matrices + A on patches, and the exact linear field from the solve."""
    g = pa.StructuredTetrahedralGrid([n_side] * 3, [1.0, 1.0, 1.0])
    g.compute_geometry()
    raw = pa.grid_to_raw(g)
    nc, nf = g.num_cells, g.num_faces
    Kvals = pa.SecondOrderTensor(np.ones(nc)).values
    bf = g.get_all_boundary_faces()
    flags = np.zeros(nf, dtype=np.uint8)
    flags[bf] = 1
    bv = np.zeros(nf)
    bv[bf] = g.face_centers[0, bf]
    # reference = True: on this lattice the reference drops exact zeros -- its stored pattern must be a subset of the
    # structural stencil, the values agree to 1e-10
    out = grid_patch_parity(lib, raw, Kvals, flags, 1.0 / 3.0, bv, np.zeros(nc), patch_targets(raw, n_random),
                            reference=True)
    out["max_abs_error_vs_exact_linear_field"] = float(np.max(np.abs(out["x"] - g.cell_centers[0])))
    return out


def full_size_patch_parity_mpsa(lib, n_side: int = 44, seeds=(0, None, -1)):
    """The same for the elasticity path at BASELINE configs[3] (511 104 tetrahedra, 1.53 M dofs):
    stress / bound_stress rows of the full problem against the MPSA oracle on patches, the exact
    uniaxial solution, the true residual."""
    from porepy_amd import distributed as D

    n = n_side
    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    g = pa.perturb_interior_nodes(g, 0.2 / n)
    nc, nf, nd = g.num_cells, g.num_faces, 3
    rng = np.random.default_rng(6)
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
    raw = pa.grid_to_raw(g)
    ctx = pa.Context(0, lib)
    ctx.set_grid(raw)
    eta = 1.0 / 3.0
    ctx.mpsa_set_params(C.values, g.cell_volumes, bc.is_dir, bc.is_neu, eta)
    ctx.mpsa_discretize()
    ctx.mpsa_assemble(bv.ravel("F"), None)
    u, info = ctx.solve("bicgstab", rtol=1e-11, maxit=50000, n=nd * nc, precond="amg")
    cc = g.cell_centers
    E, nu = 2.5, 0.25
    exact = np.vstack((nu * cc[0] / E, nu * cc[1] / E, -cc[2] / E))
    assert np.max(np.abs(u.reshape(3, -1, order="F") - exact)) < 1e-9
    A = ctx.matrix(pa._lib.MAT_MECH_SYSTEM)
    b = ctx.active_rhs(nd * nc)
    assert np.linalg.norm(b - A @ u) <= 1e-10 * np.linalg.norm(b)
    stress = ctx.matrix(MPSA_WHICH["stress"])
    bstress = ctx.matrix(MPSA_WHICH["bound_stress"])
    cn = g.cell_nodes().tocsc()
    nodes_cells = cn.tocsr()
    checked = 0
    for seed in seeds:
        c0 = {0: 0, -1: nc - 1}.get(seed, int(rng.integers(nc)))
        inner = np.unique(nodes_cells[cn.indices[cn.indptr[c0]: cn.indptr[c0 + 1]]].indices)
        owner = np.ones(nc, dtype=np.int32)
        owner[inner] = 0
        lp = D.extract_subdomain(raw, owner, 0)
        art = lp.artificial_boundary
        ldir = bc.is_dir[:, lp.face_gid].copy()
        lneu = bc.is_neu[:, lp.face_gid].copy()
        ldir[:, art] = False
        lneu[:, art] = True
        ora = so.discretize(lp.raw, np.ascontiguousarray(C.values[:, :, lp.cell_gid]), {"is_dir": ldir, "is_neu": lneu}, eta=eta)
        lcf = lp.raw["cf_indices"][: lp.raw["cf_indptr"][lp.n_own]]
        lfaces = np.unique(lcf)
        gfaces = lp.face_gid[lfaces]
        ex = lambda idx: (nd * np.asarray(idx)[:, None] + np.arange(nd)[None, :]).ravel()  # noqa: E731
        cmap = np.full(nd * nc, -1)
        cmap[ex(lp.cell_gid)] = np.arange(nd * lp.cell_gid.size)
        fmap = np.full(nd * nf, -1)
        fmap[ex(lp.face_gid)] = np.arange(nd * lp.face_gid.size)
        for name, M, m in (("stress", stress, cmap), ("bound_stress", bstress, fmap)):
            G = M[ex(gfaces)].tocoo()
            assert np.all(m[G.col] >= 0), name
            Gl = sps_csr((G.data, (G.row, m[G.col])), shape=(nd * gfaces.size, ora[name].shape[1]))
            assert rel_max_err(Gl, ora[name][ex(lfaces)]) < TOL, (name, seed)
        checked += lfaces.size
    return {"iterations": info["iterations"], "rows_checked": checked}


def morton_numbered_grid_solve(lib, n=8):
    """A grid whose cells are already numbered along the Morton curve of their centres is solved in place
    (no renumbered copy of the system, reorder.inc); any other numbering goes through the copy.  Both
    must give the solution of the direct solver."""
    from porepy_amd import distributed as D

    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    g = pa.perturb_interior_nodes(g, 0.02)
    rng = np.random.default_rng(3)
    sc = np.exp(0.5 * rng.standard_normal(g.num_cells))
    K = pa.SecondOrderTensor(kxx=sc, kyy=4 * sc, kzz=0.3 * sc, kxy=0.3 * sc)
    raw0 = pa.grid_to_raw(g)
    bf = g.get_all_boundary_faces()
    dirf = bf[(g.face_centers[0, bf] < 1e-9) | (g.face_centers[0, bf] > 1 - 1e-9)]
    flags = np.zeros(g.num_faces, dtype=np.uint8)
    flags[bf] = 2
    flags[dirf] = 1
    bv = np.zeros(g.num_faces)
    bv[dirf] = g.face_centers[0, dirf]
    its = {}
    for name in ("generator", "morton"):
        box = (raw0["face_centers"].min(axis=1), raw0["face_centers"].max(axis=1))
        order = np.arange(g.num_cells) if name == "generator" else D.morton_order(raw0["cell_centers"], 3, box)
        raw = D.permute_cells(raw0, order)
        ctx = pa.Context(0, lib)
        ctx.set_grid(raw)
        ctx.set_params(np.ascontiguousarray(K.values[:, :, order]), flags, None, 1.0 / 3.0)
        ctx.discretize(skip_vector_source=True)
        src = raw["cell_volumes"]
        ctx.assemble(bv, None, src)
        A, b = ctx.matrix(pa._lib.MAT_SYSTEM), ctx.rhs()
        xo = spla.spsolve(A.tocsc(), b)
        for precond in ("jacobi", "amg"):
            x, info = ctx.solve("bicgstab", rtol=1e-12, maxit=5000, precond=precond)
            assert info["converged"], (name, precond)
            assert np.linalg.norm(x - xo) <= TOL * np.linalg.norm(xo), (name, precond)
            its[name, precond] = info["iterations"]
            assert ctx.stats()["solve_renumbered"] == (1 if name == "generator" else 0), name
    return its


class TpfaAdCase:
    """tests/golden/tpfaad_*.npz: t_f_full and its Jacobian w.r.t. k_c from the reference's forward AD."""

    def __init__(self, name: str):
        import os

        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
        self.grid = {k[5:]: (z[k] if z[k].shape else z[k].item()) for k in z.files if k.startswith("grid_")}
        self.grid["dim"] = int(self.grid["dim"])
        self.perm = z["perm"]
        self.t_face = z["ref_t_face"]
        self.dt_dk = sps_csr((z["ref_dt_dk_data"], z["ref_dt_dk_indices"], z["ref_dt_dk_indptr"]),
                                    shape=tuple(z["ref_dt_dk_shape"]))
        self.hf_face, self.hf_cell, self.hf_sign = z["ref_hf_face"], z["ref_hf_cell"], z["ref_hf_sign"]
        self.t_half_face_inv = z["ref_t_half_face_inv"]


def check_tpfa_ad_case(lib, name: str):
    """pfv_tpfa_transmissibility_ad through the host mirror against the reference's AD result."""
    c = TpfaAdCase(name)
    g = pa.grid_from_raw(c.grid)
    d = pa.DifferentiableTpfa(library=lib)
    nc = g.num_cells
    k_c = np.ascontiguousarray(c.perm.reshape(9, nc).T).ravel()  # the reference's vector form
    t, jac = d.transmissibility(g, k_c)
    assert np.max(np.abs(t - c.t_face)) <= TOL * np.max(np.abs(c.t_face))
    assert abs(jac - c.dt_dk).max() <= TOL * abs(c.dt_dk).max()
    t2, jac2 = d.transmissibility(g, c.perm)                       # (3, 3, Nc) form
    assert np.array_equal(t, t2) and abs(jac - jac2).max() == 0.0
    fi, ci, sg = d.half_face_cells(g)
    to_ref = np.lexsort((ci, fi))  # the reference's half-face order: face by face
    assert np.array_equal(fi[to_ref], c.hf_face) and np.array_equal(ci[to_ref], c.hf_cell)
    assert np.array_equal(sg[to_ref], c.hf_sign)


def check_ad_flux_system(lib, n=3, seed=0, with_vs=True):
    """pfv_mpfa_ad_flux_system against the numpy restatement of the reference's differentiable MPFA flux
    (oracle/ad_flux_oracle.py): fluxes, dq/dp, the Jacobian J = d(div q)/dp left as the active system and the
    residual; then one Newton increment through pfv_solve against the direct solve."""
    from oracle import ad_flux_oracle as ao

    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    g = pa.perturb_interior_nodes(g, 0.1 / n, seed=seed)
    raw = pa.grid_to_raw(g)
    rng = np.random.default_rng(seed)
    nc, nf = g.num_cells, g.num_faces
    p = rng.random(nc)
    # K(p) = K0 exp(a p): d K / d p = a K
    a = 0.7
    base = pa.SecondOrderTensor(kxx=1 + rng.random(nc), kyy=2 + rng.random(nc), kzz=0.5 + rng.random(nc),
                                kxy=0.2 * rng.random(nc), kyz=0.1 * rng.random(nc)).values
    K = base * np.exp(a * p)[None, None, :]
    dk = a * K
    bf = g.get_all_boundary_faces()
    fc = g.face_centers
    dirf = bf[(fc[0, bf] < 1e-9) | (fc[0, bf] > 1 - 1e-9)]
    flags = np.zeros(nf, dtype=np.uint8)
    flags[bf] = 2
    flags[dirf] = 1
    bv = np.zeros(nf)
    bv[dirf] = 1.0 + fc[1, dirf]
    neuf = np.setdiff1d(bf, dirf)
    bv[neuf] = 0.01 * rng.random(neuf.size)
    vs = rng.random(3 * nc) if with_vs else None
    src = 0.1 * rng.random(nc)
    ctx = pa.Context(0, lib)
    ctx.set_grid(raw)
    ctx.set_params(K, flags, None, 1.0 / 3.0)
    ctx.discretize()
    mats = {"flux": ctx.matrix(WHICH["flux"]), "vector_source": ctx.matrix(WHICH["vector_source"])}
    q = ctx.ad_flux_system(p, dk, bv, vs, src, flux_jacobian=True)
    J = ctx.matrix(pa._lib.MAT_SYSTEM)
    mr = ctx.rhs()
    dq = ctx.matrix(pa._lib.MAT_FLUX_JACOBIAN)
    qo, dqo, Jo, ro = ao.flux_system(raw, mats, K, dk, p, flags, bv, vs, src)
    assert np.max(np.abs(q - qo)) <= TOL * np.max(np.abs(qo))
    assert rel_max_err(dq, dqo) < TOL
    assert rel_max_err(J, Jo) < TOL
    assert np.max(np.abs(mr + ro)) <= TOL * np.max(np.abs(ro))
    # finite-difference check of the two-point part of the oracle itself: d t_f / d p
    x, info = ctx.solve("bicgstab", rtol=1e-13, maxit=2000, precond="jacobi")
    xo = spla.spsolve(Jo.tocsc(), -ro)
    assert np.linalg.norm(x - xo) <= 1e-9 * np.linalg.norm(xo)
    # K independent of p: J is A itself, and the MPFA assembly after it is intact
    q2 = ctx.ad_flux_system(p, None, bv, vs, src)
    J2 = ctx.matrix(pa._lib.MAT_SYSTEM)
    ctx.assemble(bv, vs, src)
    A = ctx.matrix(pa._lib.MAT_SYSTEM)
    assert rel_max_err(J2, A) < 1e-14 and np.allclose(q2, q, rtol=0, atol=1e-13 * np.max(np.abs(q)))
    return {"iterations": info["iterations"], "nnz_J": int(J.nnz)}


class AdFluxCase:
    """tests/golden/adflux_*.npz: darcy_flux (value, Jacobian) of the reference's AdTpfaFlux with an Mpfa base."""

    def __init__(self, name: str):
        import os

        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
        self.grid = {k[5:]: (z[k] if z[k].shape else z[k].item()) for k in z.files if k.startswith("grid_")}
        self.grid["dim"] = int(self.grid["dim"])
        self.perm, self.dk_dp, self.p = z["perm"], z["dk_dp"], z["p"]
        self.bc_flags, self.bc_values, self.vector_source = z["bc_flags"], z["bc_values"], z["vector_source"]
        if not np.any(self.vector_source):
            self.vector_source = None

        def csr(key):
            return sps_csr((z[key + "_data"], z[key + "_indices"], z[key + "_indptr"]), shape=tuple(z[key + "_shape"]))
        self.ref_flux, self.ref_div_flux = z["ref_flux"], z["ref_div_flux"]
        self.ref_flux_jac, self.ref_div_flux_jac = csr("ref_flux_jac"), csr("ref_div_flux_jac")
        self.ref_mpfa_flux, self.ref_mpfa_vs = csr("ref_mpfa_flux"), csr("ref_mpfa_vector_source")


def check_ad_flux_case(lib, name: str):
    """pfv_mpfa_ad_flux_system (MPFA discretization of K(p) on the device + two-point product rule) against
    the reference's forward AD."""
    c = AdFluxCase(name)
    ctx = pa.Context(0, lib)
    ctx.set_grid(c.grid)
    eta = pa.determine_eta(pa.grid_from_raw(c.grid))
    ctx.set_params(c.perm, c.bc_flags, None, eta)
    ctx.discretize()
    assert rel_max_err(ctx.matrix(WHICH["flux"]), c.ref_mpfa_flux) < TOL
    q = ctx.ad_flux_system(c.p, c.dk_dp, c.bc_values, c.vector_source, None, flux_jacobian=True)
    assert np.max(np.abs(q - c.ref_flux)) <= TOL * np.max(np.abs(c.ref_flux))
    assert rel_max_err(ctx.matrix(pa._lib.MAT_FLUX_JACOBIAN), c.ref_flux_jac) < TOL
    assert rel_max_err(ctx.matrix(pa._lib.MAT_SYSTEM), c.ref_div_flux_jac) < TOL
    assert np.max(np.abs(ctx.rhs() + c.ref_div_flux)) <= TOL * np.max(np.abs(c.ref_div_flux))


def amg_robustness_sweep(lib, scale: float = 1.0):
    """The aggregation-AMG-preconditioned BiCGStab on systems that are NOT the benchmark's (its cycle
    constants were tuned there): isotropic and anisotropic Laplacians, a log-normal permeability with a
    contrast of ~1e7, a channelised 2-D field, hexahedra and tetrahedra, and a plain 7-point system handed
    over as CSR.  Returns {name: (unknowns, iterations, true relative residual)}."""
    import scipy.sparse as sps

    def n_(x):
        return max(4, int(round(x * scale)))

    def solve_grid(g, K, all_dir=False):
        bf = g.get_all_boundary_faces()
        xf = g.face_centers[0, bf]
        dirf = bf if all_dir else bf[(xf < 1e-9) | (xf > g.nodes[0].max() - 1e-9)]
        flags = np.zeros(g.num_faces, dtype=np.uint8)
        flags[bf] = 2
        flags[dirf] = 1
        bv = np.zeros(g.num_faces)
        bv[dirf] = 1.0 + g.face_centers[1, dirf]
        ctx = pa.Context(0, lib)
        ctx.set_grid(pa.grid_to_raw(g))
        ctx.set_params(K.values, flags, None, pa.determine_eta(g))
        ctx.discretize(skip_vector_source=True)
        ctx.assemble(bv, None, g.cell_volumes)
        x, info = ctx.solve("bicgstab", rtol=1e-10, maxit=2000, precond="amg", raise_on_fail=False)
        b = ctx.rhs()
        res = float(np.linalg.norm(b - ctx.spmv(pa._lib.MAT_SYSTEM, x)) / np.linalg.norm(b))
        return g.num_cells, info["iterations"], res

    def geo(g):
        g.compute_geometry()
        return g

    out = {}
    rng = np.random.default_rng(11)
    g = geo(pa.CartGrid([n_(48)] * 3, [1, 1, 1]))
    out["hex_isotropic_laplacian"] = solve_grid(g, pa.SecondOrderTensor(np.ones(g.num_cells)), all_dir=True)
    g = pa.perturb_interior_nodes(geo(pa.StructuredTetrahedralGrid([n_(20)] * 3, [1, 1, 1])), 0.2 / n_(20))
    nc = g.num_cells
    # axis-aligned anisotropy 10 : 1.  (At 100 : 1 on these perturbed tetrahedra the MPFA-O matrix has lost its
    # M-matrix structure -- 37 % positive off-diagonal entries, diagonal / off-diagonal row sums down to 1e-2 --
    # and at 48 000 cells BiCGStab breaks down and GMRES(50) stagnates with EITHER preconditioner
    # (tools/amg_aniso.py): a property of the O-method on skewed cells that the reference meets with its direct
    # solvers; the library reports PFV_ERR_NOT_CONVERGED, it does not return a wrong field.)
    out["tet_anisotropic_10"] = solve_grid(g, pa.SecondOrderTensor(kxx=np.ones(nc), kyy=np.ones(nc), kzz=0.1 * np.ones(nc)))
    sc = np.exp(2.5 * rng.standard_normal(nc))
    out["tet_lognormal_sigma2.5"] = solve_grid(g, pa.SecondOrderTensor(kxx=sc, kyy=sc, kzz=sc, kxy=0.3 * sc))
    g = geo(pa.CartGrid([n_(300), n_(300)], [1, 1]))
    k = np.ones(g.num_cells)
    yc = g.cell_centers[1]
    k[(np.abs(yc - 0.3) < 0.03) | (np.abs(yc - 0.7) < 0.02)] = 1e4
    out["quad2d_channels_1e4"] = solve_grid(g, pa.SecondOrderTensor(k))
    m = n_(64)
    e = np.ones(m)
    T = sps.diags([-e[:-1], 2 * e, -e[:-1]], [-1, 0, 1])
    eye = sps.identity(m)
    A = (sps.kron(sps.kron(T, eye), eye) + sps.kron(sps.kron(eye, T), eye) + sps.kron(sps.kron(eye, eye), T)).tocsr()
    b = rng.random(A.shape[0])
    ctx = pa.Context(0, lib)
    ctx.set_system(A, b)
    x, info = ctx.solve("bicgstab", rtol=1e-10, maxit=2000, precond="amg", raise_on_fail=False)
    out["csr_7point_laplacian"] = (A.shape[0], info["iterations"], float(np.linalg.norm(b - A @ x) / np.linalg.norm(b)))
    return out


def mpsa_patch_parity_all_matrices(lib, n_side: int = 44, n_random: int = 4, reference: bool = False):
    """BASELINE configs[3] (MPSA elasticity, rollers + top traction, perturbed tetrahedra) at full size: all FOUR
    device matrices (stress, bound_stress, bound_displacement_cell, bound_displacement_face) and the system matrix
    on patches (8 box corners -- where roller, traction and free faces meet --, 6 side centres, random cells) against
    the MPSA oracle, rows fetched with pfv_get_matrix_rows."""
    n = n_side
    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    g = pa.perturb_interior_nodes(g, 0.2 / n)
    nc, nf, nd = g.num_cells, g.num_faces, 3
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
    raw = pa.grid_to_raw(g)
    ctx = pa.Context(0, lib)
    ctx.set_grid(raw)
    eta = 1.0 / 3.0
    ctx.mpsa_set_params(C.values, g.cell_volumes, bc.is_dir, bc.is_neu, eta)
    ctx.mpsa_discretize()
    ctx.mpsa_assemble(bv.ravel("F"), None)
    cutter = PatchCutter(raw)
    ex = lambda idx: (nd * np.asarray(idx)[:, None] + np.arange(nd)[None, :]).ravel()  # noqa: E731
    worst, checked = {}, 0
    ref_inputs, ref_rows = [], []
    targets = patch_targets(raw, n_random, seed=6)
    for c0 in targets:
        inner = cutter.cells_around(c0)
        lraw, n_own, cell_gid, face_gid, art = cutter.cut(inner)
        ldir = bc.is_dir[:, face_gid].copy()
        lneu = bc.is_neu[:, face_gid].copy()
        ldir[:, art] = False
        lneu[:, art] = True
        ora = so.discretize(lraw, np.ascontiguousarray(C.values[:, :, cell_gid]), {"is_dir": ldir, "is_neu": lneu}, eta=eta)
        lfaces = np.unique(lraw["cf_indices"][: lraw["cf_indptr"][n_own]])
        gfaces = face_gid[lfaces]
        cmap = np.full(nd * nc, -1)
        cmap[ex(cell_gid)] = np.arange(nd * cell_gid.size)
        fmap = np.full(nd * nf, -1)
        fmap[ex(face_gid)] = np.arange(nd * face_gid.size)
        if reference:
            ref_inputs.append((lraw, np.ascontiguousarray(C.values[:, :, cell_gid]), {"is_dir": ldir, "is_neu": lneu}, eta))
            ref_rows.append({"rows": ex(lfaces)})
        for k in MPSA_KEYS:
            m = cmap if k in ("stress", "bound_displacement_cell") else fmap
            G = ctx.matrix_rows(MPSA_WHICH[k], ex(gfaces)).tocoo()
            assert np.all(m[G.col] >= 0), (k, c0)
            Gl = sps_csr((G.data, (G.row, m[G.col])), shape=(nd * gfaces.size, ora[k].shape[1]))
            if reference:
                ref_rows[-1][k] = Gl.copy()
            err = rel_max_err(Gl, ora[k][ex(lfaces)])
            worst[k] = max(worst.get(k, 0.0), err)
            assert err < TOL, (k, c0, err)
        checked += lfaces.size
    out = {"patches": len(targets), "rows_checked": checked, "worst_rel_err": worst}
    if reference:
        # ---- the same rows against the REFERENCE ITSELF: pp.Mpsa (numerics/fv/mpsa.py:121-529, python inverter) run on
        # the same patches with the same geometry arrays and stiffness tensors
        refs = reference_on_patches(ref_inputs, product=bool(lib.pfv_is_device_build()), keys=MPSA_KEYS)
        out["reference_patches"] = 0 if refs is None else len(refs)
        if refs is not None:
            worst_ref = {}
            for rows, ref in zip(ref_rows, refs):
                for k in MPSA_KEYS:
                    Rl = sps_csr(ref[k][rows["rows"]])
                    err = rel_max_err(rows[k], Rl)
                    worst_ref[k] = max(worst_ref.get(k, 0.0), err)
                    assert err < TOL, ("reference", k, err)
                    # what the reference stores is stored here (its sparse products drop exact zeros: subset)
                    stored = lambda mm: sps_csr((np.ones(mm.indices.size, np.int8), mm.indices, mm.indptr), shape=mm.shape)  # noqa: E731
                    Gs, Rs = sps_csr(rows[k]), Rl
                    Gs.sort_indices(); Rs.sort_indices()
                    Dm = stored(Rs) - stored(Gs)
                    assert Dm.nnz == 0 or Dm.max() <= 0, ("the reference stores an entry the device pattern lacks", k)
            out["worst_rel_err_vs_reference"] = worst_ref
    return out


def split_matches_one_piece(lib, g, K, bc, bv, split_kwargs, monkeypatch=None, free=None):
    import scipy.sparse.linalg as spla

    one = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "bc_values": bv})
    d1 = pa.Mpfa("flow", library=lib)
    d1.discretize(g, one)
    A1, b1 = d1.assemble_matrix_rhs(g, one)
    if monkeypatch is not None:
        monkeypatch.setattr(pa._lib.Context, "free_device_bytes", lambda self: free)
    many = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "bc_values": bv, **split_kwargs})
    d2 = pa.Mpfa("flow", library=lib)
    d2.discretize(g, many)
    assert id(g) in d2._split and id(g) not in d2._contexts  # no whole-grid handle was created
    m1, m2 = one[pa.DISCRETIZATION_MATRICES]["flow"], many[pa.DISCRETIZATION_MATRICES]["flow"]
    for name in ("flux", "bound_flux", "bound_pressure_cell", "bound_pressure_face", "vector_source",
                 "bound_pressure_vector_source"):
        ref = m1[name]
        assert m2[name].shape == ref.shape
        assert abs(m2[name] - ref).max() <= 1e-12 * max(abs(ref).max(), 1e-300), name
    A2, b2 = d2.assemble_matrix_rhs(g, many)
    assert abs(A2 - A1).max() <= 1e-12 * abs(A1).max()
    assert np.linalg.norm(b2 - b1) <= 1e-12 * np.linalg.norm(b1)
    x, info = d2.solve(g, many, rtol=1e-12)
    xo = spla.spsolve(A1.tocsc(), b1)
    assert info["converged"] and np.linalg.norm(x - xo) <= 1e-8 * np.linalg.norm(xo)
    assert np.array_equal(many[pa.PARAMETERS]["flow"]["active_faces"], np.arange(g.num_faces))


def mpsa_split_matches_one_piece(lib, g, C, bc, bv, split_kwargs, source=None):
    """Mpsa with partition_arguments (mpsa.py:201-207, 245-380): merged matrices, system and solution equal the
    one-piece discretization."""
    def mk(**extra):
        p = {"fourth_order_tensor": C, "bc": bc, "bc_values": bv, **extra}
        if source is not None:
            p["source"] = source
        return pa.initialize_data({}, "mechanics", p)

    one = mk()
    d1 = pa.Mpsa("mechanics", library=lib)
    d1.discretize(g, one)
    A1, b1 = d1.assemble_matrix_rhs(g, one)
    many = mk(**split_kwargs)
    d2 = pa.Mpsa("mechanics", library=lib)
    d2.discretize(g, many)
    assert id(g) in d2._split and id(g) not in d2._contexts
    m1, m2 = one[pa.DISCRETIZATION_MATRICES]["mechanics"], many[pa.DISCRETIZATION_MATRICES]["mechanics"]
    for name in MPSA_KEYS:
        ref = m1[name]
        assert m2[name].shape == ref.shape
        assert abs(m2[name] - ref).max() <= 1e-11 * max(abs(ref).max(), 1e-300), name
    A2, b2 = d2.assemble_matrix_rhs(g, many)
    assert abs(A2 - A1).max() <= 1e-11 * abs(A1).max()
    assert np.linalg.norm(b2 - b1) <= 1e-11 * max(np.linalg.norm(b1), 1e-300)
    x, info = d2.solve(g, many, rtol=1e-12)
    xo = spla.spsolve(A1.tocsc(), b1)
    assert info["converged"] and np.linalg.norm(x - xo) <= 1e-7 * np.linalg.norm(xo)


def mpsa_pieces_case(lib, dim: int):
    rng = np.random.default_rng(4)
    if dim == 3:
        g = pa.StructuredTetrahedralGrid([3, 3, 3], [1.0, 1.0, 1.0])
        g.compute_geometry()
        g = pa.perturb_interior_nodes(g, 0.03, seed=2)
    else:
        g = pa.CartGrid([7, 6], [1.0, 1.0])
        g.compute_geometry()
    nc, nf = g.num_cells, g.num_faces
    C = pa.FourthOrderTensor(1 + rng.random(nc), 0.5 + rng.random(nc))
    bc = pa.BoundaryConditionVectorial(g)
    bf = g.get_all_boundary_faces()
    bot = bf[g.face_centers[dim - 1, bf] < 1e-9]
    bc.is_dir[:, bot] = True
    bc.is_neu[:, bot] = False
    west = bf[g.face_centers[0, bf] < 1e-9]
    bc.is_dir[0, west] = True
    bc.is_neu[0, west] = False
    bv = np.zeros((dim, nf))
    top = bf[g.face_centers[dim - 1, bf] > 1 - 1e-9]
    bv[dim - 1, top] = -g.face_areas[top]
    bv[0, bot] = 0.01 * g.face_centers[0, bot]
    mpsa_split_matches_one_piece(lib, g, C, bc, bv.ravel("F"), dict(partition_arguments={"num_subproblems": 3}),
                                 source=0.01 * rng.standard_normal(dim * nc))


def hub_tetrahedral_grid(n_ring: int = 40, seed: int = 3):
    """Delaunay grid with one node met by ~40 cells / ~60 faces (more than any lattice subdivision has)."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((3, n_ring))
    u /= np.linalg.norm(u, axis=0)
    pts = np.hstack([np.zeros((3, 1)), 0.5 * u, rng.standard_normal((3, 30)) / 2]) + 0.5
    g = pa.TetrahedralGrid(pts)
    g.compute_geometry()
    return g


def mpsa_large_interaction_region(lib):
    """An unstructured grid whose hub node has a 3 x 63 = 189-unknown interaction region: too large for the LDS
    of a CU (the limit is ~36 faces per node), so it is worked on in global-memory scratch; all four matrices
    against the oracle."""
    g = hub_tetrahedral_grid()
    raw = pa.grid_to_raw(g)
    nsf_node = np.bincount(raw["fn_indices"], minlength=g.num_nodes)
    assert nsf_node.max() > 40
    nd, nc, nf = 3, g.num_cells, g.num_faces
    rng = np.random.default_rng(8)
    C = pa.FourthOrderTensor(1 + rng.random(nc), 0.5 + rng.random(nc))
    bf = g.get_all_boundary_faces()
    is_dir = np.zeros((nd, nf), bool)
    is_neu = np.zeros((nd, nf), bool)
    is_neu[:, bf] = True
    low = bf[g.face_centers[2, bf] < np.median(g.face_centers[2, bf])]
    is_dir[:, low] = True
    is_neu[:, low] = False
    ctx = pa.Context(0, lib)
    ctx.set_grid(raw)
    eta = mo.default_eta(raw["name"])
    ctx.mpsa_set_params(C.values, g.cell_volumes, is_dir, is_neu, eta)
    ctx.mpsa_discretize()
    ora = so.discretize(raw, C.values, {"is_dir": is_dir, "is_neu": is_neu}, eta=eta)
    for k in MPSA_KEYS:
        M = ctx.matrix(MPSA_WHICH[k])
        assert np.array_equal(M.indptr, ora[k].indptr) and np.array_equal(M.indices, ora[k].indices), k
        assert rel_max_err(M, ora[k]) < 1e-8, (k, rel_max_err(M, ora[k]))  # sliver cells: conditioning, not a bug
    ctx.close()


def mpfa_large_interaction_region(lib, n_ring: int = 70):
    """MPFA on a Delaunay grid whose hub node is met by more than 64 sub-faces: beyond the register Gauss-Jordan
    (one lane per row of a 64-lane wavefront), through the LDS elimination; all six matrices against the oracle."""
    g = hub_tetrahedral_grid(n_ring=n_ring, seed=5)
    raw = pa.grid_to_raw(g)
    assert np.bincount(raw["fn_indices"], minlength=g.num_nodes).max() > 64
    rng = np.random.default_rng(12)
    nc = g.num_cells
    k = 1 + rng.random(nc)
    K = pa.SecondOrderTensor(kxx=k, kyy=2 * k, kzz=0.5 * k, kxy=0.2 * k, kxz=0.05 * k, kyz=0.1 * k)
    bf = g.get_all_boundary_faces()
    low = bf[g.face_centers[2, bf] < np.median(g.face_centers[2, bf])]
    bc = pa.BoundaryCondition(g, low, ["dir"] * low.size)
    ctx = pa.Context(0, lib)
    ctx.set_grid(raw)
    eta = mo.default_eta(raw["name"])
    ctx.set_params(K.values, pa.bc_flags(bc), None, eta)
    ctx.discretize()
    ora = mo.discretize(raw, K.values, pa.bc_to_raw(bc), eta=eta)
    for i, kname in enumerate(mo.MATRIX_KEYS):
        M = ctx.matrix(i)
        assert np.array_equal(M.indptr, ora[kname].indptr) and np.array_equal(M.indices, ora[kname].indices), kname
        assert rel_max_err(M, ora[kname]) < 1e-8, (kname, rel_max_err(M, ora[kname]))  # sliver cells
    # ... and the system of this unstructured grid through assembly and the AMG-preconditioned solve
    bv = np.zeros(g.num_faces)
    bv[low] = 1.0 + g.face_centers[0, low]
    ctx.assemble(bv, None, 0.1 * g.cell_volumes)
    A = ctx.matrix(pa._lib.MAT_SYSTEM)
    b = ctx.rhs()
    x, info = ctx.solve("bicgstab", rtol=1e-12, maxit=5000, raise_on_fail=False, precond="amg")
    xo = spla.spsolve(A.tocsc(), b)
    assert info["converged"], info
    assert np.linalg.norm(x - xo) <= 1e-7 * np.linalg.norm(xo)
    ctx.close()


def biot_pieces_case(lib, name: str = "biot_tet_2x2x2_mixed", nparts: int = 3):
    """Biot with partition_arguments: the four MPSA matrices and the five coupling terms per coupling tensor equal
    the one-piece discretization."""
    c = BiotCase(name)
    g = pa.grid_from_raw(c.grid)

    def run(**extra):
        bc = pa.BoundaryConditionVectorial(g)
        bc.is_dir, bc.is_neu, bc.is_rob = c.bc["is_dir"].copy(), c.bc["is_neu"].copy(), c.bc["is_rob"].copy()
        bc.robin_weight = c.bc["robin_weight"]
        C = type("C", (), {"values": c.stiffness})()
        maps = {k: type("A", (), {"values": v})() for k, v in c.alphas.items()}
        data = pa.initialize_data({}, "mechanics", {"fourth_order_tensor": C, "bc": bc,
                                                    "scalar_vector_mappings": maps, **extra})
        d = pa.Biot("mechanics", library=lib)
        d.discretize(g, data)
        return d, data[pa.DISCRETIZATION_MATRICES]["mechanics"]

    _, one = run()
    d2, many = run(partition_arguments={"num_subproblems": nparts})
    assert id(g) not in d2._contexts  # no whole-grid handle
    for k in MPSA_KEYS:
        assert many[k].shape == one[k].shape
        assert abs(many[k] - one[k]).max() <= 1e-11 * max(abs(one[k]).max(), 1e-300), k
    for k in BIOT_KEYS:
        for key in c.alphas:
            A, B = many[k][key], one[k][key]
            assert A.shape == B.shape, (k, key)
            assert abs(A - B).max() <= 1e-11 * max(abs(B).max(), 1e-300), (k, key)


def sliver_refinement(lib):
    """Fixtures made from the reference on Delaunay SLIVER grids (oracle/gen_golden_sliver.py): the plain condensed
    solves are off by more than 1e-8 there (shown with the refinement switched off), the iterative-refinement path
    of the node kernels (mpfa_numeric.inc: kRefineKappa) brings every matrix within the 1e-10 gate."""
    def errs(mode):
        old = os.environ.get("PFV_NODE_REFINE")
        os.environ["PFV_NODE_REFINE"] = mode
        try:
            c = Case("sliver_delaunay_mixed")
            ctx = run_case(lib, c)
            e1 = max(rel_max_err(ctx.matrix(WHICH[k]), c.ref[k]) for k in ALL_KEYS)
            ctx.close()
            m = MpsaCase("mpsa_sliver_delaunay")
            ctx = run_mpsa_case(lib, m)
            e2 = max(rel_max_err(ctx.matrix(MPSA_WHICH[k]), m.ref[k]) for k in MPSA_KEYS)
            ctx.close()
        finally:
            if old is None:
                os.environ.pop("PFV_NODE_REFINE", None)
            else:
                os.environ["PFV_NODE_REFINE"] = old
        return e1, e2

    off, on = errs("-1"), errs("0")
    # the fixtures do exercise the path: without it both are an order of magnitude beyond the 1e-10 gate (how far
    # beyond is rounding noise times a condition number of ~1e7: 2e-8 ... 3e-9 from build to build)
    assert off[0] > 1e-9 and off[1] > 1e-9, off
    assert on[0] < SLIVER_TOL and on[1] < SLIVER_TOL and max(on) < 0.05 * min(off), (on, off)
    return off, on


def _geo2(g):
    g.compute_geometry()
    return g


def batch_matches_single(lib):
    """``Mpfa.discretize_batch``: grids of a mixed-dimensional model discretized as disjoint unions (one device
    discretization per dimension and continuity point) leave, grid by grid, the BITS of the single-grid path -- planes
    tilted differently in 3-D with a 3-D vector source, a plane with the default ambient dimension, Cartesian and
    simplex grids (different continuity points: separate unions), a grid with conditions per sub-face (taken alone)."""
    import scipy.sparse as sps

    rng = np.random.default_rng(5)

    def tilt(g, axis, angle, shift):
        c, s_ = np.cos(angle), np.sin(angle)
        R = {0: np.array([[1, 0, 0], [0, c, -s_], [0, s_, c]]), 1: np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])}[axis]
        g.nodes = R @ g.nodes + np.asarray(shift, float)[:, None]
        g.compute_geometry()
        return g

    def bc_for(g, sub=False):
        bf = g.get_all_boundary_faces()
        lo = bf[np.argsort(g.face_centers[0, bf] + 0.37 * g.face_centers[1, bf] + 0.11 * g.face_centers[2, bf])[: max(2, bf.size // 3)]]
        return pa.BoundaryCondition(g, lo, ["dir"] * lo.size)

    def tensor(g, full3=False):
        nc = g.num_cells
        sc = np.exp(0.4 * rng.standard_normal(nc))
        if g.dim == 3 or full3:
            return pa.SecondOrderTensor(kxx=sc, kyy=3 * sc, kzz=0.5 * sc, kxy=0.3 * sc, kyz=0.1 * sc, kxz=0.05 * sc)
        return pa.SecondOrderTensor(kxx=sc, kyy=3 * sc, kxy=0.3 * sc)

    grids = [
        (tilt(_geo2(pa.CartGrid([5, 4], [1.0, 1.0])), 0, 0.7, [0.1, 0.2, 0.3]), {"ambient_dimension": 3}, True),
        (tilt(_geo2(pa.CartGrid([3, 6], [0.5, 1.0])), 1, -0.4, [1.0, 0.0, 0.2]), {"ambient_dimension": 3}, True),
        (_geo2(pa.CartGrid([4, 4], [1.0, 2.0])), {}, False),
        (tilt(_geo2(pa.StructuredTriangleGrid([3, 3], [1.0, 1.0])), 0, 1.1, [0.0, 0.5, 0.0]), {"ambient_dimension": 3}, True),
        (_geo2(pa.StructuredTriangleGrid([4, 2], [2.0, 1.0])), {}, False),
        (_geo2(pa.CartGrid([3, 3, 2], [1.0, 1.0, 1.0])), {}, False),
        (_geo2(pa.CartGrid([2, 3, 3], [1.0, 2.0, 1.0])), {}, False),
        (pa.perturb_interior_nodes(_geo2(pa.StructuredTetrahedralGrid([2, 2, 2], [1.0, 1.0, 1.0])), 0.05), {}, False),
    ]
    items_b, items_s = [], []
    for g, extra, full3 in grids:
        K = tensor(g, full3)
        bc = bc_for(g)
        for items in (items_b, items_s):
            items.append((g, pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc,
                                                             "bc_values": np.zeros(g.num_faces), **extra})))
    db, ds = pa.Mpfa("flow", library=lib), pa.Mpfa("flow", library=lib)
    stats = db.discretize_batch(items_b)
    # unions: 2-D Cartesian (eta 0: 3 grids), 2-D triangles (eta 1/3: 2), 3-D Cartesian (2); the tetrahedral grid is alone
    assert stats == {"unions": 3, "batched": 7, "single": 1}, stats
    for (g, dat_b), (_, dat_s) in zip(items_b, items_s):
        ds.discretize(g, dat_s)
        mb, ms = dat_b[pa.DISCRETIZATION_MATRICES]["flow"], dat_s[pa.DISCRETIZATION_MATRICES]["flow"]
        for k in ALL_KEYS:
            a, b = sps.csr_matrix(mb[k]), sps.csr_matrix(ms[k])
            assert a.shape == b.shape, (g.name, k, a.shape, b.shape)
            assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices), (g.name, k)
            assert np.array_equal(a.data, b.data), (g.name, k, float(abs(a - b).max()))
        assert np.array_equal(dat_b[pa.PARAMETERS]["flow"]["active_faces"], np.arange(g.num_faces))
        # the system of a grid that was part of a union assembles like any other
        Ab, bb = db.assemble_matrix_rhs(g, dat_b)
        As, bs_ = ds.assemble_matrix_rhs(g, dat_s)
        assert rel_max_err(Ab, As) < 1e-14 and np.allclose(bb, bs_, rtol=0, atol=1e-14)
        # ... also with a vector source (ambient coordinates for the planes discretized with ambient_dimension 3:
        # the union's matrices carry the lift already, the split path must not project the source a second time)
        vdim = dat_b[pa.PARAMETERS]["flow"].get("ambient_dimension", g.dim)
        vs = np.random.default_rng(11 + g.num_cells).standard_normal(vdim * g.num_cells)
        dat_b[pa.PARAMETERS]["flow"]["vector_source"] = vs
        dat_s[pa.PARAMETERS]["flow"]["vector_source"] = vs.copy()
        Ab, bb = db.assemble_matrix_rhs(g, dat_b)
        As, bs_ = ds.assemble_matrix_rhs(g, dat_s)
        assert float(np.abs(bs_).max()) > 0.0
        assert rel_max_err(Ab, As) < 1e-14 and np.allclose(bb, bs_, rtol=0, atol=1e-13 * max(1.0, float(np.abs(bs_).max()))), g.name
        xb, _ = db.solve(g, dat_b, rtol=1e-12)
        xs, _ = ds.solve(g, dat_s, rtol=1e-12)
        assert np.allclose(xb, xs, rtol=0, atol=1e-8 * max(1.0, float(np.abs(xs).max()))), g.name
    return stats


def batch_hands_special_inputs_to_the_single_grid_path(lib):
    """A pair with a partial specification, or with a per-sub-face continuity point, is not laid into a union: it goes
    through ``discretize`` as if called alone; the others still share one device discretization."""
    def grid(nx, ny):
        g = pa.CartGrid([nx, ny], [1.0, 1.0])
        g.compute_geometry()
        return g

    def data_for(g, **extra):
        bf = g.get_all_boundary_faces()
        bc = pa.BoundaryCondition(g, bf[:4], ["dir"] * 4)
        K = pa.SecondOrderTensor(kxx=np.linspace(1.0, 2.0, g.num_cells), kyy=np.full(g.num_cells, 3.0))
        return pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "bc_values": np.zeros(g.num_faces), **extra})

    gs = [grid(4, 3), grid(3, 3), grid(5, 2), grid(4, 4)]
    extras = [{}, {}, {"specified_cells": np.array([0, 1])}, {"mpfa_eta": np.full(int(gs[3].face_nodes.nnz), 0.1)}]
    items = [(g, data_for(g, **e)) for g, e in zip(gs, extras)]
    d = pa.Mpfa("flow", library=lib)
    stats = d.discretize_batch(items)
    assert stats == {"unions": 1, "batched": 2, "single": 2}, stats
    for (g, dat), e in zip(items, extras):
        ref = data_for(g, **e)
        pa.Mpfa("flow", library=lib).discretize(g, ref)
        for k in ALL_KEYS:
            a, b = dat[pa.DISCRETIZATION_MATRICES]["flow"][k].tocsr(), ref[pa.DISCRETIZATION_MATRICES]["flow"][k].tocsr()
            assert a.shape == b.shape and abs(a - b).max() == 0.0, (g.num_cells, k)
    assert items[2][1][pa.PARAMETERS]["flow"]["active_faces"].size < gs[2].num_faces  # (the partial one stayed partial)
    return stats


# ------------------------------------------------------------------------------------ MPSA, whole-grid value datum
def mpsa_whole_grid_problem(n: int):
    """The problem of oracle/gen_golden_mpsa_whole_grid.py (the BASELINE configs[3] family: perturbed tetrahedral box,
    rollers on the low faces, traction on top) with heterogeneous Lame parameters: (grid, mu, lambda, is_dir, is_neu,
    boundary values face-major)."""
    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    g = pa.perturb_interior_nodes(g, 0.2 / n)
    nc, nf = g.num_cells, g.num_faces
    rng = np.random.default_rng(5)
    mu, lam = np.exp(0.3 * rng.standard_normal(nc)), np.exp(0.3 * rng.standard_normal(nc))
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
    bv[0, top] = 0.3 * g.face_areas[top]  # (a shear component: the field is not the uniaxial one)
    return g, mu, lam, np.asarray(bc.is_dir, bool), np.asarray(bc.is_neu, bool), bv.ravel("F")


def mpsa_stress_rows_that_count(raw, is_neu):
    """Rows (nd * face + component) of ``stress`` outside the Neumann components of boundary faces: there the true
    entries are all zero and what either side stores is cancellation noise (as the Neumann rows of ``flux``)."""
    nd = int(raw["dim"])
    nf = raw["face_centers"].shape[1]
    sides = np.bincount(np.asarray(raw["cf_indices"]), minlength=nf)
    noise = (sides == 1)[None, :] & np.asarray(is_neu, bool)
    return ~noise.ravel("F")


def mpsa_whole_grid_check(lib, n: int = 16):
    """All four MPSA matrices and the displacement field on the WHOLE grid against a run of the reference on it
    (tests/golden/mpsawhole_<n>.npz): block digests of the values (bench.value_digest), norm and block sums of u."""
    import json

    import bench

    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"mpsawhole_{n}.npz"))
    info = json.loads(str(z["info"]))
    g, mu, lam, is_dir, is_neu, bvf = mpsa_whole_grid_problem(n)
    assert g.num_cells == info["cells"]
    C = pa.FourthOrderTensor(mu, lam)
    ctx = pa.Context(0, lib)
    try:
        ctx.set_grid(pa.grid_to_raw(g))
        ctx.mpsa_set_params(C.values, g.cell_volumes, is_dir, is_neu, 1.0 / 3.0)
        ctx.mpsa_discretize(rebuild_topology=True)
        ctx.mpsa_assemble(bvf, None)
        u, sol = ctx.solve("bicgstab", rtol=1e-13, maxit=50000, n=3 * g.num_cells, raise_on_fail=False, precond="amg")
        mats = {k: ctx.matrix(MPSA_WHICH[k]) for k in MPSA_KEYS}
    finally:
        ctx.close()
    out = {"cells": int(g.num_cells), "iterations": int(sol["iterations"]), "rel_residual": float(sol["rel_residual"]),
           "reference": info}
    blocks = z["stress_digest"].shape[1]
    for k in MPSA_KEYS:
        mask = mpsa_stress_rows_that_count(pa.grid_to_raw(g), is_neu) if k == "stress" else None
        dev, ref = bench.value_digest(mats[k], blocks, rows_mask=mask), z[k + "_digest"]
        scale = np.maximum(np.abs(ref[0]), 1e-300)
        out[k] = [float(np.max(np.abs(dev[0] - ref[0]) / scale)),
                  float(np.max(np.abs(dev[1] - ref[1]) / np.maximum(np.abs(ref[1]), 1e-300))),
                  float(np.max(np.abs(dev[2] - ref[2]) / scale))]
        assert mats[k].nnz >= info["nnz"][k], (k, mats[k].nnz, info["nnz"][k])  # (the reference drops exact zeros)
    out["u_norm_rel_diff"] = float(abs(np.linalg.norm(u) - z["u_norm"][0]) / z["u_norm"][0])
    ud, ur = bench.vector_digest(u, blocks), z["u_digest"]
    out["u_block_squares_worst_rel_diff"] = float(np.max(np.abs(ud[1] - ur[1]) / np.maximum(ur[1], 1e-300)))
    # the fine datum (oracle/gen_golden_mpsa_fine.py): per block of 256 rows sum |a| and max |a| of the reference's matrices
    fine = os.path.join(os.path.dirname(__file__), "golden", f"mpsawhole_fine_{n}.npz")
    if os.path.exists(fine):
        zf = np.load(fine)
        assert json.loads(str(zf["info"]))["cells"] == g.num_cells
        worst_sum = worst_max = 0.0
        blocks_checked = 0
        for k in MPSA_KEYS:
            mask = mpsa_stress_rows_that_count(pa.grid_to_raw(g), is_neu) if k == "stress" else None
            dev, ref = bench.fine_digest(mats[k], rows_mask=mask), zf[k + "_fine"]
            assert dev.shape == ref.shape, (k, dev.shape, ref.shape)
            nz = ref[0] > 0.0
            assert np.all(dev[0][~nz] <= 1e-13 * np.max(ref[0])), k  # (blocks the reference leaves empty stay empty)
            worst_sum = max(worst_sum, float(np.max(np.abs(dev[0][nz] - ref[0][nz]) / ref[0][nz])))
            worst_max = max(worst_max, float(np.max(np.abs(dev[1][nz] - ref[1][nz]) / ref[1][nz])))
            blocks_checked += int(nz.sum())
        out["fine"] = {"blocks_of_256_rows": blocks_checked, "worst_rel_diff_of_block_sums": worst_sum,
                       "worst_rel_diff_of_block_maxima": worst_max}
    return out


# ------------------------------------------------------------------------------------ Biot, whole-grid value datum
def biot_whole_grid_alpha(nc: int):
    """(3, 3, Nc) coupling tensor of oracle/gen_golden_biot_whole_grid.py: heterogeneous, anisotropic, symmetric."""
    rng = np.random.default_rng(6)
    a = np.zeros((3, 3, nc))
    a[0, 0], a[1, 1], a[2, 2] = 0.6 + 0.4 * rng.random(nc), 0.5 + 0.5 * rng.random(nc), 0.7 + 0.3 * rng.random(nc)
    a[0, 1] = a[1, 0] = 0.1 * rng.random(nc)
    a[0, 2] = a[2, 0] = 0.05 * rng.random(nc)
    a[1, 2] = a[2, 1] = 0.08 * rng.random(nc)
    return a


def biot_whole_grid_check(lib, n: int = 16):
    """The five Biot coupling matrices (and stress / bound_stress) on the WHOLE grid against a run of the reference's
    pp.Biot on it (tests/golden/biotwhole_<n>.npz): block digests of the values (bench.value_digest)."""
    import json

    import bench
    from tests._golden import BIOT_KEYS

    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"biotwhole_{n}.npz"))
    info = json.loads(str(z["info"]))
    g, mu, lam, is_dir, is_neu, _ = mpsa_whole_grid_problem(n)
    assert g.num_cells == info["cells"]
    bc = pa.BoundaryConditionVectorial(g)
    bc.is_dir, bc.is_neu = is_dir.copy(), is_neu.copy()
    al = type("A", (), {"values": biot_whole_grid_alpha(g.num_cells)})()
    data = pa.initialize_data({}, "mechanics", {"fourth_order_tensor": pa.FourthOrderTensor(mu, lam), "bc": bc,
                                               "mpsa_eta": 1.0 / 3.0, "scalar_vector_mappings": {"pressure": al}})
    pa.Biot("mechanics", library=lib).discretize(g, data)
    md = data[pa.DISCRETIZATION_MATRICES]["mechanics"]
    rows = mpsa_stress_rows_that_count(pa.grid_to_raw(g), is_neu)
    blocks = z["stress_digest"].shape[1]
    out = {"cells": int(g.num_cells), "reference": info}

    def worst(dev, ref):
        scale = np.maximum(np.abs(ref[0]), 1e-300)
        return [float(np.max(np.abs(dev[0] - ref[0]) / scale)),
                float(np.max(np.abs(dev[1] - ref[1]) / np.maximum(np.abs(ref[1]), 1e-300))),
                float(np.max(np.abs(dev[2] - ref[2]) / scale))]

    for k in BIOT_KEYS:
        M = md[k]["pressure"]
        assert list(M.shape) == info["shapes"][k], (k, M.shape)
        out[k] = worst(bench.value_digest(M, blocks, rows_mask=rows if k == "scalar_gradient" else None), z[k + "_digest"])
    out["stress"] = worst(bench.value_digest(md["stress"], blocks, rows_mask=rows), z["stress_digest"])
    out["bound_stress"] = worst(bench.value_digest(md["bound_stress"], blocks), z["bound_stress_digest"])
    return out


def symbolic_reuse_on_rebuilt_topology(lib, n=4):
    """A discretization with ``rebuild_topology=True`` always rebuilds the sub-cell topology; the CSR patterns, column
    maps and face records are kept when the rebuilt topology is PROVED equal (digest + sizes) to the one they were built
    from (``pfv_stats.symbolic_reused``), and rebuilt on every miss: another grid, another boundary, ``PFV_SYMB_REUSE=0``.
    Kept or rebuilt, the matrices must be the same bits (the pattern) and the same values as a cold handle's."""
    M = pa._lib
    keys = (M.MAT_FLUX, M.MAT_BOUND_FLUX, M.MAT_BOUND_PRESSURE_CELL, M.MAT_BOUND_PRESSURE_FACE, M.MAT_VECTOR_SOURCE,
            M.MAT_BOUND_PRESSURE_VECTOR_SOURCE)

    def problem(nn, seed, all_dir=False):
        g = pa.StructuredTetrahedralGrid([nn, nn, nn], [1.0, 1.0, 1.0])
        g.compute_geometry()
        g = pa.perturb_interior_nodes(g, 0.03)
        rng = np.random.default_rng(seed)
        sc = np.exp(0.7 * rng.standard_normal(g.num_cells))
        K = pa.SecondOrderTensor(kxx=sc, kyy=3 * sc, kzz=0.5 * sc, kxy=0.2 * sc, kyz=0.1 * sc)
        bf = g.get_all_boundary_faces()
        flags = np.zeros(g.num_faces, dtype=np.uint8)
        flags[bf] = 2
        dirf = bf if all_dir else bf[g.face_centers[0, bf] < 1e-9]
        flags[dirf] = 1
        return pa.grid_to_raw(g), np.ascontiguousarray(K.values), flags

    def mats(ctx):
        out = [ctx.matrix(k) for k in keys]
        return out

    def same(a, b, exact_values):
        for x, y in zip(a, b):
            assert np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices)
            if exact_values:
                assert np.array_equal(x.data, y.data)

    raw, K1, flags = problem(n, 1)
    _, K2, _ = problem(n, 2)
    cold = pa.Context(0, lib)
    cold.set_grid(raw)
    cold.set_params(K2, flags, None, 1.0 / 3.0)
    cold.discretize()
    ref2 = mats(cold)
    assert cold.stats()["symbolic_reused"] == 0

    ctx = pa.Context(0, lib)
    ctx.set_grid(raw)
    ctx.set_params(K1, flags, None, 1.0 / 3.0)
    ctx.discretize(rebuild_topology=True)
    assert ctx.stats()["symbolic_reused"] == 0          # first call: nothing to keep
    ctx.set_params(K2, flags, None, 1.0 / 3.0)          # new values, same grid
    ctx.discretize(rebuild_topology=True)
    st = ctx.stats()
    assert st["symbolic_reused"] == 1, st
    same(mats(ctx), ref2, exact_values=True)            # kept patterns, the cold handle's bits
    ctx.assemble(np.zeros(raw["face_centers"].shape[1]), None, raw["cell_volumes"])
    cold.assemble(np.zeros(raw["face_centers"].shape[1]), None, raw["cell_volumes"])
    A1, A2 = ctx.matrix(M.MAT_SYSTEM), cold.matrix(M.MAT_SYSTEM)
    assert np.array_equal(A1.indices, A2.indices) and np.array_equal(A1.data, A2.data)
    # div @ flux under kept patterns: the first assembly records where every flux entry lands in A's rows, the next ones
    # replay the positions (device build; simplices / hexahedra) -- the same bits either way
    ctx.discretize(rebuild_topology=True)
    ctx.assemble(np.zeros(raw["face_centers"].shape[1]), None, raw["cell_volumes"])
    st = ctx.stats()
    assert st["symbolic_reused"] == 1
    if lib.pfv_is_device_build() == 1:
        assert st["assemble_positions_kept"] == 1, st
    A3 = ctx.matrix(M.MAT_SYSTEM)
    assert np.array_equal(A3.indices, A2.indices) and np.array_equal(A3.data, A2.data)
    assert np.array_equal(ctx.rhs(), cold.rhs())

    # other condition TYPES on the same boundary: the patterns do not depend on them -> still kept
    _, _, flags_d = problem(n, 1, all_dir=True)
    ctx.set_params(K2, flags_d, None, 1.0 / 3.0)
    ctx.discretize(rebuild_topology=True)
    assert ctx.stats()["symbolic_reused"] == 1
    cold_d = pa.Context(0, lib)
    cold_d.set_grid(raw)
    cold_d.set_params(K2, flags_d, None, 1.0 / 3.0)
    cold_d.discretize()
    same(mats(ctx), mats(cold_d), exact_values=True)

    # the switch: never keep
    os.environ["PFV_SYMB_REUSE"] = "0"
    try:
        ctx.discretize(rebuild_topology=True)
        assert ctx.stats()["symbolic_reused"] == 0
        same(mats(ctx), mats(cold_d), exact_values=True)
    finally:
        del os.environ["PFV_SYMB_REUSE"]
    ctx.discretize(rebuild_topology=True)
    assert ctx.stats()["symbolic_reused"] == 0          # (patterns built under the switch carry no key: rebuilt once more)
    ctx.discretize(rebuild_topology=True)
    assert ctx.stats()["symbolic_reused"] == 1
    same(mats(ctx), mats(cold_d), exact_values=True)

    # another grid on the same handle: a miss, and the right matrices
    raw3, K3, flags3 = problem(n + 1, 3)
    ctx.set_grid(raw3)
    ctx.set_params(K3, flags3, None, 1.0 / 3.0)
    ctx.discretize(rebuild_topology=True)
    assert ctx.stats()["symbolic_reused"] == 0
    cold3 = pa.Context(0, lib)
    cold3.set_grid(raw3)
    cold3.set_params(K3, flags3, None, 1.0 / 3.0)
    cold3.discretize()
    same(mats(ctx), mats(cold3), exact_values=True)
    return True


def check_mpsa_contrast_case(lib, name: str):
    """Stiffness contrasts of 1e8 ... 1e12 between cells sharing a node: the interaction regions beyond
    1e6 are assembled and eliminated in double-double (``pfv_stats.mpsa_contrast_regions`` says how many).  The device must
    be within 1e-10 of the matrices the reference's own local systems have in 60-digit arithmetic -- and of the matrices
    ``pp.Mpsa`` returned wherever those are themselves that close to the exact ones (beyond ~1e10 the reference's FP64
    inverse is the side that is off, by 1e-7 on the tetrahedral 1e12 fixture).  With ``PFV_MPSA_DD=0`` (the FP64 body on
    every region: the round-5 state) the same comparison must FAIL on at least one fixture: the test of the test."""
    from tests._golden import MpsaContrastCase

    c = MpsaContrastCase(name)

    def run():
        ctx = pa.Context(0, lib)
        ctx.set_grid(c.grid)
        ctx.mpsa_set_params(c.stiffness, c.grid["cell_volumes"], c.bc["is_dir"], c.bc["is_neu"], mo.default_eta(c.grid["name"]))
        ctx.mpsa_discretize()
        mats = {k: ctx.matrix(MPSA_WHICH[k]) for k in MPSA_KEYS}
        st = ctx.stats()
        ctx.close()
        return mats, st

    mats, st = run()
    assert st["mpsa_contrast_regions"] > 0, st
    assert st["mpsa_max_contrast"] >= 10.0 ** (c.decades - 1.5), st
    worst = 0.0
    for k in MPSA_KEYS:
        e_exact = rel_max_err(mats[k], c.exact[k])
        worst = max(worst, e_exact)
        assert e_exact < 1e-10, (name, k, "vs exact", e_exact)
        e_ref = rel_max_err(mats[k], c.ref[k])
        assert e_ref < max(1e-10, 4.0 * c.ref_off_exact[k]), (name, k, "vs reference", e_ref, c.ref_off_exact[k])
    return worst


def mpsa_contrast_fp64_body_misses(lib):
    """The same fixtures with the double-double body switched off: the FP64 condensed system loses eps x contrast."""
    from tests._golden import MpsaContrastCase, mpsa_contrast_case_names

    os.environ["PFV_MPSA_DD"] = "0"
    try:
        worst = 0.0
        for name in mpsa_contrast_case_names():
            c = MpsaContrastCase(name)
            ctx = pa.Context(0, lib)
            ctx.set_grid(c.grid)
            ctx.mpsa_set_params(c.stiffness, c.grid["cell_volumes"], c.bc["is_dir"], c.bc["is_neu"], mo.default_eta(c.grid["name"]))
            try:
                ctx.mpsa_discretize()
            except pa.PorefvError:
                worst = max(worst, 1.0)  # ("singular" where the reference returns: the other face of the same loss)
                continue
            assert ctx.stats()["mpsa_contrast_regions"] > 0   # (counted although not treated: the fence)
            for k in MPSA_KEYS:
                worst = max(worst, rel_max_err(ctx.matrix(MPSA_WHICH[k]), c.exact[k]))
            ctx.close()
        return worst
    finally:
        del os.environ["PFV_MPSA_DD"]


def implicit_vector_source_pattern(lib, n=4):
    """Beyond 2^31 entries (~6.3 M tetrahedra on one handle) the two vector-source matrices keep no CSR arrays of their own:
    values addressed through the flux pattern, products by ``spmv_vs_implicit``, exports by rows.  ``PFV_VS_IMPLICIT=1``
    forces that form at any size: every route must return what the explicit form returns -- exported matrices bit for
    bit (whole and by rows), the product and the right-hand side with a vector source to rounding; the whole-matrix C
    export is refused with the message that names the row export."""
    M = pa._lib
    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    g = pa.perturb_interior_nodes(g, 0.03)
    rng = np.random.default_rng(8)
    sc = np.exp(0.5 * rng.standard_normal(g.num_cells))
    K = pa.SecondOrderTensor(kxx=sc, kyy=2 * sc, kzz=0.4 * sc, kxy=0.2 * sc, kxz=0.1 * sc)
    bf = g.get_all_boundary_faces()
    flags = np.zeros(g.num_faces, dtype=np.uint8)
    flags[bf] = 2
    flags[bf[g.face_centers[2, bf] < 1e-9]] = 1
    raw = pa.grid_to_raw(g)
    gvec = rng.standard_normal(3 * g.num_cells)
    bv = rng.standard_normal(g.num_faces) * (flags > 0)
    out = {}
    saved = os.environ.get("PFV_VS_IMPLICIT")
    try:
        for mode in ("0", "1"):
            os.environ["PFV_VS_IMPLICIT"] = mode
            ctx = pa.Context(0, lib)
            ctx.set_grid(raw)
            ctx.set_params(np.ascontiguousarray(K.values), flags, None, 1.0 / 3.0)
            ctx.discretize()
            vs = ctx.matrix(M.MAT_VECTOR_SOURCE)
            bpvs = ctx.matrix(M.MAT_BOUND_PRESSURE_VECTOR_SOURCE)
            some = np.array([0, 3, g.num_faces - 1, 7])
            part = ctx.matrix_rows(M.MAT_VECTOR_SOURCE, some)
            only = ctx.matrix(M.MAT_VECTOR_SOURCE, rows=some)
            y = ctx.spmv(M.MAT_VECTOR_SOURCE, gvec) if hasattr(ctx, "spmv") else None
            ctx.assemble(bv, gvec, g.cell_volumes)
            b = ctx.rhs()
            if mode == "1":
                nnz = ctx.matrix_info(M.MAT_VECTOR_SOURCE)[2]
                ip = np.zeros(g.num_faces + 1, np.int32)
                ix = np.zeros(nnz, np.int32)
                dv = np.zeros(nnz)
                with pytest_raises(pa.PorefvError) as e:
                    ctx._check(ctx.lib.pfv_get_matrix(ctx._h, M.MAT_VECTOR_SOURCE, M._ptr(ip, M._ip), M._ptr(ix, M._ip), M._ptr(dv, M._dp)))
                assert "pfv_get_matrix_rows" in str(e.value)
            out[mode] = (vs, bpvs, part, only, y, b)
            ctx.close()
    finally:
        if saved is None:
            os.environ.pop("PFV_VS_IMPLICIT", None)
        else:
            os.environ["PFV_VS_IMPLICIT"] = saved
    a, b = out["0"], out["1"]
    for i in range(4):
        assert a[i].shape == b[i].shape
        assert np.array_equal(a[i].indptr, b[i].indptr) and np.array_equal(a[i].indices, b[i].indices)
        assert np.array_equal(a[i].data, b[i].data)
    if a[4] is not None:
        assert np.linalg.norm(a[4] - b[4]) <= 1e-14 * np.linalg.norm(a[4])
    assert np.linalg.norm(a[5] - b[5]) <= 1e-13 * np.linalg.norm(a[5])
    assert np.linalg.norm(a[5] - (g.cell_volumes - g.cell_faces.T @ (0 * bv))) > 0  # (the vector source did reach the rhs)
    return True


def pytest_raises(exc):
    import pytest

    return pytest.raises(exc)


def mpsa_assemble_positions_replayed(lib, n=5):
    """``div @ stress`` under kept patterns: the first assembly records the position of every stress entry in the rows of the
    mechanics system, the following ones replay them (device build) -- same matrix, same right-hand side, bit for bit."""
    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    g = pa.perturb_interior_nodes(g, 0.04)
    nc, nf = g.num_cells, g.num_faces
    rng = np.random.default_rng(12)
    bc = pa.BoundaryConditionVectorial(g)
    bf = g.get_all_boundary_faces()
    for axis in range(3):
        roll = bf[g.face_centers[axis, bf] < 1e-9]
        bc.is_dir[axis, roll] = True
        bc.is_neu[axis, roll] = False
    bv = rng.standard_normal((3, nf)) * (bc.is_dir | bc.is_neu)
    ctx = pa.Context(0, lib)
    ctx.set_grid(pa.grid_to_raw(g))
    out = []
    for k in range(3):
        C = pa.FourthOrderTensor(1.0 + rng.random(nc), 1.0 + rng.random(nc)) if k < 2 else C  # noqa: F821 (third = second field again)
        ctx.mpsa_set_params(C.values, g.cell_volumes, bc.is_dir, bc.is_neu, 1.0 / 3.0)
        ctx.mpsa_discretize(rebuild_topology=True)
        ctx.mpsa_assemble(bv.ravel("F"), None)
        out.append((ctx.matrix(pa._lib.MAT_MECH_SYSTEM), ctx.active_rhs(3 * nc), int(ctx.stats()["assemble_positions_kept"]),
                    int(ctx.stats()["symbolic_reused"])))
    ctx.close()
    assert [o[3] for o in out] == [0, 1, 1]
    if lib.pfv_is_device_build() == 1:
        assert [o[2] for o in out] == [0, 1, 1], [o[2] for o in out]  # (the first assembly under the key records)
    cold = pa.Context(0, lib)
    cold.set_grid(pa.grid_to_raw(g))
    cold.mpsa_set_params(C.values, g.cell_volumes, bc.is_dir, bc.is_neu, 1.0 / 3.0)
    cold.mpsa_discretize()
    cold.mpsa_assemble(bv.ravel("F"), None)
    A0, b0 = cold.matrix(pa._lib.MAT_MECH_SYSTEM), cold.active_rhs(3 * nc)
    cold.close()
    for A, b, _, _ in out[1:]:
        assert np.array_equal(A.indices, A0.indices) and np.array_equal(A.data, A0.data) and np.array_equal(b, b0)
    return True


def mpsa_singular_corner_is_an_error_not_a_fault(lib):
    """Component-wise conditions that leave a rigid mode of a boundary region free make its local system singular (the
    reference returns the inverse of rounding noise or raises; the differential driver classifies them "singular input").
    On the device such a region fails the unpivoted check, goes to the double-double body, and its pivot columns turn into
    NaNs after the zero pivot: the step must report "singular" (status 1) -- not index a row by the empty result of the
    pivot search (round 6: a GPU memory fault found by the large device fuzz, fixed in gj_wide / node_gj_lds)."""
    hits = 0
    for seed in (3, 11, 17):  # (found by search: 3 x 3 Cartesian grid, Dirichlet / Neumann per component at random)
        rng = np.random.default_rng(seed)
        g = pa.CartGrid([3, 3], [1.0, 1.0])
        g.compute_geometry()
        nc = g.num_cells
        bf = g.get_all_boundary_faces()
        bc = pa.BoundaryConditionVectorial(g)
        for a in range(2):
            tdir = rng.random(bf.size) < 0.5
            bc.is_dir[a, bf[tdir]] = True
            bc.is_neu[a, bf[tdir]] = False
            bc.is_neu[a, bf[~tdir]] = True
        C = pa.FourthOrderTensor(np.ones(nc), np.ones(nc))
        ctx = pa.Context(0, lib)
        ctx.set_grid(pa.grid_to_raw(g))
        ctx.mpsa_set_params(C.values, g.cell_volumes, bc.is_dir, bc.is_neu, 0.0)
        try:
            ctx.mpsa_discretize()
        except pa.PorefvError as e:
            hits += int(e.status == 1)
        ctx.close()
    assert hits == 3, hits
    return True
