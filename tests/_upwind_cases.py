"""Cases of the upwind discretization and the transport step (porepy_amd.Upwind, csrc/upwind.inc), shared by the
emulation suite (test_upwind_emulation.py) and the GPU suite (test_gpu_upwind.py): each takes the library to run on.

Fixtures: tests/golden/upwind/upwind_*.npz, made by tools/gen_golden_upwind.py from the reference."""
import ctypes
import glob
import os

import numpy as np
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import porepy_amd as pa
from porepy_amd import _lib
from tests._golden import check_pattern, rel_max_err

TOL = 1e-10  # the project's tolerance (tests/_parity.py: TOL)
UPWIND_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upwind")
KW = "transport"
KEYS = ("transport", "rhs_dir", "rhs_neu")


def fixture_names():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(UPWIND_DIR, "upwind_*.npz")))
    assert len(names) >= 10
    return names


class _Bc:
    def __init__(self, raw):
        self.is_dir, self.is_neu, self.is_rob = raw["is_dir"], raw["is_neu"], raw["is_rob"]
        self.is_internal, self.robin_weight = raw["is_internal"], raw["robin_weight"]


def _csr(z, prefix):
    return sps.csr_matrix((z[prefix + "_data"], z[prefix + "_indices"], z[prefix + "_indptr"]),
                          shape=tuple(int(v) for v in z[prefix + "_shape"]))


def same_csr(ours, ref, what=""):
    """Shape, indptr, indices and data equal to the reference's canonical CSR, bitwise."""
    ours = sps.csr_matrix(ours)
    assert ours.shape == ref.shape, (what, ours.shape, ref.shape)
    assert np.array_equal(ours.indptr, ref.indptr), what
    assert np.array_equal(ours.indices, ref.indices), what
    assert ours.data.tobytes() == np.asarray(ref.data, dtype=np.float64).tobytes(), what


def geo(g):
    g.compute_geometry()
    return g


def tets(n, perturb=True):
    g = geo(pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0]))
    return pa.perturb_interior_nodes(g, 0.2 / n) if perturb else g


def line_grid(n, length):
    """1-D grid of n cells on [0, length] (faces = nodes, normals along +x, areas 1): raw arrays as pp.CartGrid([n])
    has them."""
    x = np.linspace(0.0, length, n + 1)
    pts = np.vstack([x, np.zeros(n + 1), np.zeros(n + 1)])
    normals = np.vstack([np.ones(n + 1), np.zeros(n + 1), np.zeros(n + 1)])
    cc = np.vstack([0.5 * (x[1:] + x[:-1]), np.zeros(n), np.zeros(n)])
    return pa.grid_from_raw({
        "dim": 1, "name": "line", "nodes": pts, "cf_indptr": 2 * np.arange(n + 1, dtype=np.int32),
        "cf_indices": np.column_stack([np.arange(n), np.arange(1, n + 1)]).ravel().astype(np.int32),
        "cf_sign": np.tile(np.array([-1, 1], dtype=np.int8), n), "fn_indptr": np.arange(n + 2, dtype=np.int32),
        "fn_indices": np.arange(n + 1, dtype=np.int32), "face_normals": normals, "face_centers": pts.copy(),
        "cell_centers": cc, "face_areas": np.ones(n + 1), "cell_volumes": np.diff(x)})


# ---- numpy restatement of the scheme (from raw arrays) --------------------------------------------------------
def upwind_numpy(g, q, is_dir, is_neu, k=1):
    cf = sps.csc_matrix(g.cell_faces)
    nf, nc = cf.shape
    fi, ci, sg = sps.find(cf)
    side = -np.ones((2, nf), dtype=np.int64)
    side[0, fi[sg > 0]] = ci[sg > 0]
    side[1, fi[sg < 0]] = ci[sg < 0]
    with np.errstate(invalid="ignore"):
        pos = np.sign(q) >= 0
    up = np.where(pos, side[0], side[1])
    dirin = is_dir & (up < 0)
    kept = ~(is_neu | dirin)
    assert np.all(up[kept] >= 0)
    f = np.flatnonzero(kept)
    U = sps.coo_matrix((np.ones(f.size), (f, up[f])), shape=(nf, nc)).tocsr()
    sgn_div = np.asarray(cf.sum(axis=1)).ravel()
    fn, fd = np.flatnonzero(is_neu), np.flatnonzero(dirin)
    N = sps.coo_matrix((sgn_div[fn].astype(float), (fn, fn)), shape=(nf, nf)).tocsr()
    D = sps.coo_matrix((np.ones(fd.size), (fd, fd)), shape=(nf, nf)).tocsr()
    # kron(., eye(k)) as scipy forms it: a dense k x k block per stored entry, the zeros off its diagonal stored
    out = [sps.bsr_matrix((M.data[:, None, None] * np.eye(k), M.indices, M.indptr), shape=(k * M.shape[0], k * M.shape[1]))
           .tocsr() for M in (U, D, N)]
    return dict(zip(KEYS, out))


def system_numpy(g, q, mats, bc_values):
    div = sps.csr_matrix(g.cell_faces).T.tocsr()
    Q = sps.diags(q)
    A = div @ Q @ mats["transport"]
    b = div @ ((mats["rhs_neu"] + mats["rhs_dir"] @ Q) @ bc_values)
    return sps.csr_matrix(A), b


def default_flags(g):
    bf = g.get_all_boundary_faces()
    d = np.zeros(g.num_faces, dtype=bool)
    d[bf] = True
    return d, np.zeros(g.num_faces, dtype=bool)


def data_for(q, bc, bc_values, k=1):
    par = {"darcy_flux": q, "bc_values": bc_values}
    if bc is not None:
        par["bc"] = bc
    if k != 1:
        par["num_components"] = k
    return pa.initialize_data({}, KW, par)


# ---- fixture parity --------------------------------------------------------------------------------------------
def fixture_parity(lib, name):
    z = np.load(os.path.join(UPWIND_DIR, name + ".npz"))
    if name == "upwind_point0d":
        class Point:
            dim, num_cells, num_faces = 0, 1, 0
        data = data_for(np.zeros(0), None, np.zeros(0))
        pa.Upwind(KW, library=lib).discretize(Point(), data)
        md = data[pa.DISCRETIZATION_MATRICES][KW]
        assert [list(md[k].shape) for k in KEYS] == z["shapes"].tolist()
        return {}
    raw = {k[5:]: z[k] for k in z.files if k.startswith("grid_")}
    raw["dim"], raw["name"] = int(raw["dim"]), str(raw["name"])
    g = pa.grid_from_raw(raw)
    bc = _Bc({k[3:]: z[k] for k in z.files if k.startswith("bc_") and k != "bc_values"}) if bool(z["has_bc"]) else None
    k = int(z["num_components"])
    q = z["flux"]
    data = data_for(q, bc, z["bc_values"], k)
    up = pa.Upwind(KW, library=lib)
    assert up.ndof(g) == g.num_cells
    up.discretize(g, data)
    md = data[pa.DISCRETIZATION_MATRICES][KW]
    for key in KEYS:
        same_csr(md[key], _csr(z, "ref_" + key), (name, key))
    # the numpy restatement agrees with the reference too (it judges the grids that have no fixture)
    is_dir, is_neu = (bc.is_dir, bc.is_neu) if bc is not None else default_flags(g)
    mine = upwind_numpy(g, q, is_dir, is_neu, k)
    for key in KEYS:
        same_csr(mine[key], _csr(z, "ref_" + key), (name, key, "numpy restatement"))
    out = {}
    if k != 1:
        try:
            up.assemble_matrix_rhs(g, data)
        except ValueError:
            return out
        raise AssertionError("assembly with two components must raise ValueError")
    A, b = up.assemble_matrix_rhs(g, data)
    Aref, bref = _csr(z, "ref_A"), z["ref_rhs"]
    subset, outside, _ = check_pattern(A, Aref)
    out["A_err"] = rel_max_err(A, Aref)
    out["rhs_err"] = float(np.abs(b - bref).max() / max(np.abs(bref).max(), 1e-300))
    print(f"{name}: A rel_max_err {out['A_err']:.2e}, outside pattern {outside:.2e}, rhs {out['rhs_err']:.2e}")
    assert subset and outside <= 1e-12
    assert out["A_err"] <= TOL and out["rhs_err"] <= TOL
    if "flow_p" in z.files:  # case 5: the flux itself from the resident MPFA discretization
        K = pa.SecondOrderTensor.__new__(pa.SecondOrderTensor)
        K.values = z["flow_perm"]
        fbc = _Bc({kk[7:]: z[kk] for kk in z.files if kk.startswith("flowbc_")})
        fdata = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": fbc, "bc_values": z["flow_bc_values"]})
        mp = pa.Mpfa("flow", library=lib)
        mp.discretize(g, fdata)
        qd = mp.darcy_flux(g, fdata, z["flow_p"])
        out["q_err"] = float(np.abs(qd - q).max() / np.abs(q).max())
        print(f"{name}: face flux error {out['q_err']:.2e} of max|q|")
        assert out["q_err"] <= TOL
    return out


def nan_goes_to_the_negative_branch(lib):
    g = geo(pa.CartGrid([4, 3], [4.0, 3.0]))
    rng = np.random.default_rng(5)
    q = rng.random(g.num_faces) - 0.5
    interior = np.setdiff1d(np.arange(g.num_faces), g.get_all_boundary_faces())
    q[interior[[0, 3, 7]]] = np.nan
    bf = g.get_all_boundary_faces()
    q[bf[2]] = np.nan
    q[bf[-1]] = np.nan
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    data = data_for(q, bc, np.zeros(g.num_faces))
    pa.Upwind(KW, library=lib).discretize(g, data)
    ref = upwind_numpy(g, q, bc.is_dir, bc.is_neu)
    for key in KEYS:
        same_csr(data[pa.DISCRETIZATION_MATRICES][KW][key], ref[key], key)
    U = data[pa.DISCRETIZATION_MATRICES][KW]["transport"]
    cf = sps.csc_matrix(g.cell_faces)
    for f in interior[[0, 3, 7]]:
        _, cells, signs = sps.find(sps.csr_matrix(cf)[f])
        neg_cell = cells[signs < 0][0]
        assert U[f].indices.tolist() == [neg_cell]


def random_signs(lib, n):
    """A grid without a fixture: random sign pattern, mixed conditions, against the numpy restatement."""
    g = tets(n)
    rng = np.random.default_rng(n)
    q = rng.standard_normal(g.num_faces)
    q[rng.integers(0, g.num_faces, g.num_faces // 20)] = 0.0
    q[rng.integers(0, g.num_faces, g.num_faces // 20)] = -0.0
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, list(np.array(["dir", "neu", "dir"])[np.arange(bf.size) % 3]))
    bv = np.zeros(g.num_faces)
    bv[bf] = rng.random(bf.size)
    data = data_for(q, bc, bv)
    up = pa.Upwind(KW, library=lib)
    up.discretize(g, data)
    ref = upwind_numpy(g, q, bc.is_dir, bc.is_neu)
    md = data[pa.DISCRETIZATION_MATRICES][KW]
    for key in KEYS:
        same_csr(md[key], ref[key], key)
    A, b = up.assemble_matrix_rhs(g, data)
    Aref, bref = system_numpy(g, q, ref, bv)
    subset, outside, _ = check_pattern(A, Aref)
    err = rel_max_err(A, Aref)
    berr = np.abs(b - bref).max() / np.abs(bref).max()
    print(f"tets {n}^3: {g.num_cells} cells, A rel_max_err {err:.2e}, rhs {berr:.2e}")
    assert subset and outside <= 1e-12 and err <= TOL and berr <= TOL
    # the exported system is what the handle multiplies with
    x = rng.random(g.num_cells)
    y = up.context(g).spmv(_lib.MAT_TRANSPORT_SYSTEM, x)
    assert np.abs(y - Aref @ x).max() <= TOL * np.abs(Aref @ x).max()


# ---- implicit Euler ---------------------------------------------------------------------------------------------
def euler_closed_form(lib):
    n, qv, dt, phi = 16, 0.7, 0.05, 0.3
    g = line_grid(n, 2.0)
    vol = g.cell_volumes
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir", "dir"])
    q = qv * np.ones(g.num_faces)
    bv = np.zeros(g.num_faces)
    bv[0] = 1.0
    acc = phi * vol / dt
    data = data_for(q, bc, bv)
    up = pa.Upwind(KW, library=lib)
    up.discretize(g, data)
    nu = qv / acc

    def recursion(c, steps):
        for _ in range(steps):
            new = np.empty(n)
            for i in range(n):
                new[i] = (c[i] + nu[i] * (new[i - 1] if i else 1.0)) / (1 + nu[i])
            c = new
        return c

    # The issue's case: from rest, Dirichlet inflow value 1, with the default method.  (From rest the first residual is
    # one entry in the inflow cell and the matrix is lower bidiagonal: plain BiCGStab has rho = (r0, r1) = 0 after one
    # iteration; advance solves such a step again with GMRES from the kept state.)
    for method in ("bicgstab", "gmres"):
        c, info = up.advance(g, data, np.zeros(n), 10, acc, rtol=1e-13, method=method)
        assert info["steps_done"] == 10 and info["converged"], (method, info)
        err = np.abs(c - recursion(np.zeros(n), 10)).max()
        st = up.context(g).stats()
        print(f"implicit Euler, closed form (c0 = 0, {method}): max error {err:.2e}, "
              f"{st['transport_gmres_retries']} steps retried with GMRES")
        assert err <= 1e-10
    # a start that excites every cell
    c0 = 0.5 + 0.25 * np.cos(np.arange(n))
    c, info = up.advance(g, data, c0, 10, acc, rtol=1e-13)
    assert info["steps_done"] == 10 and info["converged"]
    err = np.abs(c - recursion(c0, 10)).max()
    print(f"implicit Euler, closed form (c0 generic, BiCGStab): max error {err:.2e}")
    assert err <= 1e-10
    # one step through solve() is the same step
    c1, _ = up.solve(g, data, accumulation=acc, c_old=c0, rtol=1e-13)
    assert np.abs(c1 - recursion(c0, 1)).max() <= 1e-10


def conservation_and_bounds(lib, n=4):
    g = tets(n)
    rng = np.random.default_rng(3)
    up = pa.Upwind(KW, library=lib)
    q = up.darcy_flux(g, [0.6, -0.3, 0.45])
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    bv = np.zeros(g.num_faces)
    bv[bf] = rng.random(bf.size)
    acc = 0.25 * g.cell_volumes / 0.02
    data = data_for(q, bc, bv)
    up.discretize(g, data)
    A, bref = up.assemble_matrix_rhs(g, data)
    c = rng.random(g.num_cells)
    for step in range(5):
        new, info = up.advance(g, data, c, 1, acc, rtol=1e-13)
        assert info["steps_done"] == 1
        lhs = np.sum(acc * (new - c))
        rhs = -np.sum(bref) - np.sum(A @ new)
        assert abs(lhs - rhs) <= 1e-10 * np.sum(acc), (step, lhs, rhs)
        assert new.min() >= -1e-10 and new.max() <= 1 + 1e-10, (step, new.min(), new.max())
        c = new


# ---- the resident pipeline ------------------------------------------------------------------------------------
def flow_problem(g, rng):
    nc = g.num_cells
    k = 1 + rng.random(nc)
    K = pa.SecondOrderTensor(kxx=k, kyy=1.5 * k, kzz=0.7 * k, kxy=0.1 * k)
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    bv = np.zeros(g.num_faces)
    bv[bf] = g.face_centers[:, bf].sum(axis=0)  # pressure drop along the diagonal: flux through every face region
    return pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "bc_values": bv}), bv


def resident_pipeline(lib, n, to_device, to_host, scheme="mpfa"):
    g = tets(n)
    rng = np.random.default_rng(11)
    fdata, fbv = flow_problem(g, rng)
    flow = (pa.Mpfa if scheme == "mpfa" else pa.Tpfa)("flow", library=lib)
    flow.discretize(g, fdata)
    ctx = flow.context(g)
    p, info = flow.solve(g, fdata, rtol=1e-13, **({"method": "bicgstab"} if scheme == "tpfa" else {}))
    assert info["converged"]
    # device: p and every other vector stay in device memory
    nc, nf = g.num_cells, g.num_faces
    bf = g.get_all_boundary_faces()
    tbv = np.zeros(nf)
    tbv[bf] = rng.random(bf.size)
    acc = 0.2 * g.cell_volumes / 0.05
    c0 = rng.random(nc)
    d_p, k1 = to_device(np.ascontiguousarray(p))
    d_fbv, k2 = to_device(fbv)
    d_tbv, k3 = to_device(tbv)
    d_acc, k4 = to_device(acc)
    d_c, k5 = to_device(c0.copy())
    ctx.face_flux(d_p, d_fbv, device=True)
    tdata = pa.initialize_data({}, KW, {"bc_values": tbv, "darcy_flux": pa.ResidentFlux(ctx)})
    up = pa.Upwind(KW, library=lib, flow=flow)
    assert up.context(g) is ctx
    up.discretize(g, tdata)  # default conditions: Dirichlet on the boundary; the flux is the resident one
    ctx.upwind_assemble(d_tbv, None, accumulation=d_acc, device=True)
    _, ainfo = ctx.transport_advance(d_c, 5, rtol=1e-13, device=True)
    assert ainfo["steps_done"] == 5
    c_dev = to_host(k5)
    # the Python-level chain gives the same bits
    tdata2 = pa.initialize_data({}, KW, {"bc_values": tbv})
    flow.darcy_flux(g, fdata, p, resident=True)
    up.discretize(g, tdata2)
    c_api, _ = up.advance(g, tdata2, c0, 5, acc, rtol=1e-13)
    assert np.array_equal(c_api, c_dev)
    # host: the same chain from the handle's exported matrices
    md = fdata[pa.DISCRETIZATION_MATRICES]["flow"]
    qh = md["flux"] @ p + md["bound_flux"] @ fbv
    is_dir, is_neu = default_flags(g)
    mats = upwind_numpy(g, qh, is_dir, is_neu)
    Ah, bh = system_numpy(g, qh, mats, tbv)
    M = (sps.diags(acc) + Ah).tocsc()
    ch = c0.copy()
    for _ in range(5):
        ch = spla.spsolve(M, acc * ch - bh)
    err = np.abs(c_dev - ch).max() / np.abs(ch).max()
    print(f"resident pipeline ({scheme}, {nc} cells): max-norm difference {err:.2e}")
    assert err <= 1e-10
    # the flux copied out is the resident one
    qd = flow.darcy_flux(g, fdata, p)
    assert np.abs(qd - qh).max() <= TOL * np.abs(qh).max()
    del k1, k2, k3, k4


def advection_diffusion(lib, n=4):
    g = tets(n)
    rng = np.random.default_rng(17)
    up = pa.Upwind(KW, library=lib)
    q = up.darcy_flux(g, [0.5, 0.2, -0.4])
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    bv = np.zeros(g.num_faces)
    bv[bf] = rng.random(bf.size)
    tdata = data_for(q, bc, bv)
    up.discretize(g, tdata)
    A, bref = up.assemble_matrix_rhs(g, tdata)
    ddata, _ = flow_problem(g, rng)
    ddata[pa.PARAMETERS]["flow"]["bc_values"] = bv
    tp = pa.Tpfa("flow", library=lib)
    tp.discretize(g, ddata)
    D, bd = tp.assemble_matrix_rhs(g, ddata)
    acc = 0.3 * g.cell_volumes / 0.1
    ctx = up.context(g)
    dA = pa.DeviceCsr.from_discretization(ctx, _lib.MAT_TRANSPORT_SYSTEM)
    dD = pa.DeviceCsr.from_discretization(tp.context(g), _lib.MAT_SYSTEM, ctx)
    dS = dA + dD + pa.DeviceCsr.from_scipy(sps.diags(acc).tocsr(), ctx)
    S = sps.csr_matrix(A) + sps.csr_matrix(D) + sps.diags(acc)
    diff = abs(dS.to_scipy() - S).max()
    assert diff <= 1e-14 * max(1.0, abs(S).max()), diff
    rhs = acc * rng.random(g.num_cells) - bref + bd
    dS.as_system(rhs)
    x, info = ctx.solve(method="bicgstab", rtol=1e-13)
    ref = spla.spsolve(S.tocsc(), rhs)
    err = np.abs(x - ref).max() / np.abs(ref).max()
    print(f"advection-diffusion: {err:.2e}")
    assert info["converged"] and err <= 1e-10


def injection_from_rest(lib, n=4):
    """A single source cell in a field at rest, divergence-free flow in 3-D: the first residual sits in one cell that
    nothing flows back into.  advance with the default method must deliver the steps (spsolve is the judge)."""
    g = tets(n)
    up = pa.Upwind(KW, library=lib)
    q = up.darcy_flux(g, [0.6, -0.3, 0.45])
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    bv = np.zeros(g.num_faces)
    acc = 0.25 * g.cell_volumes / 0.02
    src = np.zeros(g.num_cells)
    src[g.num_cells // 2] = 1.0
    data = data_for(q, bc, bv)
    up.discretize(g, data)
    A, bref = up.assemble_matrix_rhs(g, data)
    c, info = up.advance(g, data, np.zeros(g.num_cells), 3, acc, source=src, rtol=1e-13)
    assert info["steps_done"] == 3 and info["converged"], info
    M = (sps.diags(acc) + sps.csr_matrix(A)).tocsc()
    ref = np.zeros(g.num_cells)
    for _ in range(3):
        ref = spla.spsolve(M, acc * ref - bref + src)
    err = np.abs(c - ref).max() / np.abs(ref).max()
    print(f"injection from rest: {err:.2e}, retried steps {up.context(g).stats()['transport_gmres_retries']}")
    assert err <= 1e-10


def face_flux_with_vector_source(lib, scheme, dim, implicit):
    """pfv_mpfa_face_flux with a vector source, against the products of the exported matrices; ``implicit``: the
    vector-source values addressed through the flux pattern (PFV_VS_IMPLICIT=1)."""
    old = os.environ.get("PFV_VS_IMPLICIT")
    os.environ["PFV_VS_IMPLICIT"] = "1" if implicit else "0"
    try:
        g = tets(3) if dim == 3 else pa.perturb_interior_nodes(geo(pa.StructuredTriangleGrid([5, 4], [1.0, 1.0])), 0.03)
        rng = np.random.default_rng(31)
        fdata, fbv = flow_problem(g, rng)
        bf = g.get_all_boundary_faces()
        fdata[pa.PARAMETERS]["flow"]["bc"] = pa.BoundaryCondition(
            g, bf, list(np.array(["dir", "neu", "dir"])[np.arange(bf.size) % 3]))
        vs = rng.standard_normal(g.dim * g.num_cells)
        fdata[pa.PARAMETERS]["flow"]["vector_source"] = vs
        flow = (pa.Mpfa if scheme == "mpfa" else pa.Tpfa)("flow", library=lib)
        flow.discretize(g, fdata)
        p = rng.standard_normal(g.num_cells)
        q = flow.darcy_flux(g, fdata, p)
    finally:
        if old is None:
            del os.environ["PFV_VS_IMPLICIT"]
        else:
            os.environ["PFV_VS_IMPLICIT"] = old
    md = fdata[pa.DISCRETIZATION_MATRICES]["flow"]
    ref = md["flux"] @ p + md["bound_flux"] @ fbv + md["vector_source"] @ vs
    without = md["flux"] @ p + md["bound_flux"] @ fbv
    assert np.abs(ref - without).max() > 1e-3 * np.abs(ref).max()  # (the term is there)
    err = np.abs(q - ref).max() / np.abs(ref).max()
    print(f"face flux with vector source ({scheme}, {dim}-D, implicit={implicit}): {err:.2e}")
    assert err <= TOL


def stale_system_is_not_solved(lib):
    """After a new discretization (or new conditions) the transport system assembled before is gone: solve must
    refuse instead of returning the solution of the previous system."""
    import pytest

    g = geo(pa.CartGrid([4, 3], [4.0, 3.0]))
    up = pa.Upwind(KW, library=lib)
    q = up.darcy_flux(g, [1.0, 0.5, 0.0])
    bv = np.ones(g.num_faces)
    acc = np.ones(g.num_cells)
    data = data_for(q, None, bv)
    up.discretize(g, data)
    c, _ = up.solve(g, data, accumulation=acc, c_old=np.full(g.num_cells, 0.5))
    ctx = up.context(g)
    for redo in (lambda: ctx.upwind_discretize(-q, 1), lambda: ctx.upwind_set_bc(None)):
        up.discretize(g, data)
        up.solve(g, data, accumulation=acc, c_old=np.full(g.num_cells, 0.5))
        redo()
        assert ctx.active_size() == 0
        with pytest.raises(RuntimeError):
            ctx.solve()
        with pytest.raises(pa.PorefvError):
            ctx.transport_advance(np.zeros(g.num_cells), 1)


# ---- determinism, isolation, errors ---------------------------------------------------------------------------
def _run_all(lib, n, seed=23):
    g = tets(n)
    rng = np.random.default_rng(seed)
    fdata, fbv = flow_problem(g, rng)
    mp = pa.Mpfa("flow", library=lib)
    mp.discretize(g, fdata)
    p, _ = mp.solve(g, fdata, rtol=1e-12)
    q = mp.darcy_flux(g, fdata, p)
    mp.darcy_flux(g, fdata, p, resident=True)
    bf = g.get_all_boundary_faces()
    tbv = np.zeros(g.num_faces)
    tbv[bf] = rng.random(bf.size)
    up = pa.Upwind(KW, library=lib, flow=mp)
    tdata = pa.initialize_data({}, KW, {"bc_values": tbv})
    up.discretize(g, tdata)
    A, b = up.assemble_matrix_rhs(g, tdata)
    acc = 0.2 * g.cell_volumes / 0.05
    c, _ = up.advance(g, tdata, rng.random(g.num_cells), 3, acc, rtol=1e-12)
    md = tdata[pa.DISCRETIZATION_MATRICES][KW]
    return g, mp, fdata, [p, q, b, c, A.indptr, A.indices, A.data] + [a for k in KEYS for a in
                                                                     (md[k].indptr, md[k].indices, md[k].data)]


def deterministic(lib, n=4):
    _, _, _, a = _run_all(lib, n)
    _, _, _, b = _run_all(lib, n)
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def nothing_else_moves(lib, n=4):
    g, mp, fdata, _ = _run_all(lib, n)  # a handle that also ran the upwind calls
    rng = np.random.default_rng(23)
    fdata2, _ = flow_problem(tets(n), rng)
    g2 = tets(n)
    mp2 = pa.Mpfa("flow", library=lib)
    mp2.discretize(g2, fdata2)
    for k in ("flux", "bound_flux", "bound_pressure_cell", "bound_pressure_face", "vector_source",
              "bound_pressure_vector_source"):
        a = mp.context(g).matrix(getattr(_lib, "MAT_" + k.upper()))
        b = mp2.context(g2).matrix(getattr(_lib, "MAT_" + k.upper()))
        same_csr(a, b, k)
    A1, b1 = mp.assemble_matrix_rhs(g, fdata)  # (the active system is shared: assemble the flow system again)
    A2, b2 = mp2.assemble_matrix_rhs(g2, fdata2)
    same_csr(A1, A2, "A")
    assert np.asarray(b1).tobytes() == np.asarray(b2).tobytes()
    x1, i1 = mp.solve(g, fdata, rtol=1e-12)
    x2, i2 = mp2.solve(g2, fdata2, rtol=1e-12)
    assert x1.tobytes() == x2.tobytes() and i1["iterations"] == i2["iterations"]
    # offsets of the existing statistics: a read of the old struct size gives the same leading fields
    ctx = mp.context(g)
    full = _lib.Stats()
    ctx._check(ctx.lib.pfv_get_stats_n(ctx._h, ctypes.byref(full), ctypes.sizeof(full)))
    old_fields = _lib.Stats._fields_[:[n for n, _ in _lib.Stats._fields_].index("amg_nns_modes") + 1]

    class OldStats(ctypes.Structure):
        _fields_ = old_fields

    assert ctypes.sizeof(OldStats) == 34 * 8
    buf = (ctypes.c_char * (ctypes.sizeof(OldStats) + 64))()
    ctypes.memset(buf, 0x5a, len(buf))
    ctx._check(ctx.lib.pfv_get_stats_n(ctx._h, buf, ctypes.sizeof(OldStats)))
    assert bytes(buf[ctypes.sizeof(OldStats):]) == b"\x5a" * 64
    assert bytes(buf[:ctypes.sizeof(OldStats)]) == bytes(full)[:ctypes.sizeof(OldStats)]
    st = ctx.stats()
    assert st["upwind_ms"] >= 0 and st["transport_iterations"] > 0


def errors(lib):
    import pytest

    g = geo(pa.CartGrid([4, 3], [4.0, 3.0]))
    bf = g.get_all_boundary_faces()
    up = pa.Upwind(KW, library=lib)
    q = up.darcy_flux(g, [1.0, 0.5, 0.0])
    bv = np.zeros(g.num_faces)
    # assemble before discretize
    with pytest.raises(ValueError):
        up.assemble_matrix_rhs(g, data_for(q, None, bv))
    # num_components < 1
    with pytest.raises(ValueError):
        up.discretize(g, data_for(q, None, bv, k=0))
    with pytest.raises(pa.PorefvError) as e:
        up.context(g).upwind_discretize(q, 0)
    assert e.value.status == 4
    # assemble with two components
    d2 = data_for(q, None, bv, k=2)
    up.discretize(g, d2)
    with pytest.raises(ValueError):
        up.assemble_matrix_rhs(g, d2)
    # Robin face with inflow: no upstream cell
    rob = pa.BoundaryCondition(g, bf, ["rob"] * bf.size)
    with pytest.raises(ValueError, match="negative axis 1 index: -1") as e:
        up.discretize(g, data_for(q, rob, bv))
    cfd = sps.csc_matrix(g.cell_faces)
    inflow = [f for f in bf if (q[f] >= 0) != (sps.find(cfd[f])[2][0] > 0)]
    assert f"face {min(inflow)} " in str(e.value)
    # flux array of the wrong length
    with pytest.raises(ValueError):
        up.discretize(g, data_for(q[:-1], None, bv))
    # resident flux requested but none computed
    tp = pa.Tpfa("flow", library=lib)
    K = pa.SecondOrderTensor(np.ones(g.num_cells))
    fdata = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": pa.BoundaryCondition(g, bf, ["dir"] * bf.size),
                                            "bc_values": bv})
    tp.discretize(g, fdata)
    upr = pa.Upwind(KW, library=lib, flow=tp)
    with pytest.raises(ValueError):
        upr.discretize(g, pa.initialize_data({}, KW, {"bc_values": bv}))
    with pytest.raises(KeyError):
        up.discretize(g, pa.initialize_data({}, KW, {"bc_values": bv}))
    # periodic grid
    gp = geo(pa.CartGrid([3, 3], [1.0, 1.0]))
    left = np.flatnonzero(np.isclose(gp.face_centers[0], 0.0))
    right = np.flatnonzero(np.isclose(gp.face_centers[0], 1.0))
    gp.periodic_face_map = np.vstack([left, right])
    with pytest.raises(pa.PorefvError) as e:
        up.discretize(gp, data_for(np.ones(gp.num_faces), None, np.zeros(gp.num_faces)))
    assert e.value.status == 5
    # advance without accumulation on a grid with an all-inflow cell (zero diagonal)
    g1 = line_grid(6, 1.0)
    q1 = np.where(g1.face_centers[0] < 0.5, 1.0, -1.0)  # both neighbours flow into the middle cells
    d1 = data_for(q1, None, np.zeros(g1.num_faces))
    up.discretize(g1, d1)
    up.assemble_matrix_rhs(g1, d1)  # the reference's call itself is fine
    with pytest.raises(pa.PorefvError) as e:
        up.advance(g1, d1, np.zeros(6), 2, None)
    assert e.value.status == 5 and "zero diagonal" in e.value.message
