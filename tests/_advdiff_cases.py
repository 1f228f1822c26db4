"""Cases of the advection-diffusion system and its implicit Euler step (porepy_amd.AdvectionDiffusion,
csrc/advdiff.inc), shared by the emulation suite (test_advdiff_emulation.py) and the GPU suite (test_gpu_advdiff.py).
The judge is scipy on the host: S = diag(acc) + A_D + w A_U, r = acc c - b_U + b_D + source, spsolve.

Fixtures: tests/golden/advdiff/advdiff_*.npz, made by tools/gen_golden_advdiff.py from the reference."""
import glob
import os

import numpy as np
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import porepy_amd as pa
from porepy_amd import _lib
from tests._golden import check_pattern, rel_max_err
from tests._upwind_cases import _Bc, _csr, geo, line_grid, same_csr, system_numpy, tets, upwind_numpy

TOL = 1e-10  # the project's tolerance (tests/_parity.py: TOL)
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "advdiff")
KW = "transport"


def fixture_names():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "advdiff_*.npz")))
    assert len(names) >= 8
    return names


def tensor(values):
    K = pa.SecondOrderTensor.__new__(pa.SecondOrderTensor)
    K.values = np.asarray(values, dtype=float)
    return K


# ---- 1. fixture parity ------------------------------------------------------------------------------------------
def fixture_parity(lib, name):
    z = np.load(os.path.join(DIR, name + ".npz"))
    raw = {k[5:]: z[k] for k in z.files if k.startswith("grid_")}
    raw["dim"], raw["name"] = int(raw["dim"]), str(raw["name"])
    g = pa.grid_from_raw(raw)
    bc = _Bc({k[3:]: z[k] for k in z.files if k.startswith("bc_") and k != "bc_values"})
    w = float(z["flux_scale"])
    par = {"second_order_tensor": tensor(z["perm"]), "bc": bc, "bc_values": z["bc_values"], "darcy_flux": z["flux"]}
    if w != 1.0:
        par["flux_scale"] = w
    data = pa.initialize_data({}, KW, par)
    ad = pa.AdvectionDiffusion(KW, scheme="tpfa" if bool(z["tpfa"]) else "mpfa", library=lib)
    ad.discretize(g, data)
    A, b = ad.assemble_matrix_rhs(g, data)
    Aref = sps.csr_matrix(_csr(z, "ref_AD") + w * _csr(z, "ref_AU"))
    bref = z["ref_bD"] - z["ref_bUw"]
    subset, outside, _ = check_pattern(A, Aref)
    a_err = rel_max_err(A, Aref)
    b_err = float(np.abs(b - bref).max() / np.abs(bref).max())
    print(f"{name}: A rel_max_err {a_err:.2e}, outside pattern {outside:.2e}, b {b_err:.2e}")
    assert subset and outside <= 1e-12
    assert a_err <= TOL and b_err <= TOL
    # one step from the fixture's state against spsolve
    acc, c0, src = z["acc"], z["c0"], z["source"]
    c, info = ad.advance(g, data, c0, 1, acc, source=src)
    ref = spla.spsolve((sps.diags(acc) + Aref).tocsc(), acc * c0 + bref + src)
    err = np.abs(c - ref).max()
    print(f"{name}: one step, max error {err:.2e}")
    assert info["steps_done"] == 1 and err <= 1e-10


# ---- problems without a fixture: judged by the numpy restatement of the scheme -----------------------------------
def grid_of(kind):
    if kind == "quad":
        return geo(pa.CartGrid([7, 5], [7.0, 5.0]))
    if kind == "line":
        return line_grid(11, 2.0)
    return tets(int(kind[4:]))


def problem(g, seed=5, diffusivity=1.0, closed=False, velocity=(0.6, -0.3, 0.45)):
    """Parameters of one keyword on g: heterogeneous anisotropic tensor x diffusivity, mixed Dirichlet / Neumann
    boundary (closed: zero Neumann everywhere and no flux through the boundary), a constant-velocity flux."""
    rng = np.random.default_rng(seed)
    nc, nf = g.num_cells, g.num_faces
    k = diffusivity * (1 + rng.random(nc))
    K = pa.SecondOrderTensor(kxx=k, kyy=1.5 * k, kzz=0.7 * k, kxy=0.1 * k) if g.dim == 3 else (
        pa.SecondOrderTensor(kxx=k, kyy=1.5 * k, kxy=0.2 * k) if g.dim == 2 else pa.SecondOrderTensor(k))
    bf = g.get_all_boundary_faces()
    q = pa.Upwind(KW).darcy_flux(g, list(velocity))
    bv = np.zeros(nf)
    if closed:
        bc = pa.BoundaryCondition(g, bf, ["neu"] * bf.size)
        q[bf] = 0.0
    else:
        bc = pa.BoundaryCondition(g, bf, list(np.array(["dir", "neu", "dir"])[np.arange(bf.size) % 3]))
        bv[bf] = np.where(bc.is_dir[bf], 0.25 + rng.random(bf.size), 0.05 * (rng.random(bf.size) - 0.5))
    par = {"second_order_tensor": K, "bc": bc, "bc_values": bv, "darcy_flux": q}
    vol = np.asarray(g.cell_volumes, dtype=float)
    return {"par": par, "bc": bc, "bv": bv, "q": q, "acc": (0.2 + 0.3 * rng.random(nc)) * vol / 0.05,
            "c0": rng.random(nc), "src": (0.0 if closed else 0.1) * (rng.random(nc) - 0.5) * vol}


def host_system(g, md, pr, q=None, w=1.0):
    """(A, b) of the steady balance A c = b + source from the exported diffusion matrices and the numpy upwind."""
    q = pr["q"] if q is None else q
    div = sps.csr_matrix(g.cell_faces).T.tocsr()
    A_D = div @ sps.csr_matrix(md["flux"])
    b_D = -(div @ (sps.csr_matrix(md["bound_flux"]) @ pr["bv"]))
    mats = upwind_numpy(g, q, np.asarray(pr["bc"].is_dir, bool), np.asarray(pr["bc"].is_neu, bool))
    A_U, b_U = system_numpy(g, w * q, mats, pr["bv"])
    return sps.csr_matrix(A_D + A_U), b_D - b_U


def host_steps(A, b, acc, c, src, n):
    M = (sps.diags(acc) + A).tocsc()
    for _ in range(n):
        c = spla.spsolve(M, acc * c + b + src)
    return c


def discretized(lib, g, pr, scheme="mpfa"):
    data = pa.initialize_data({}, KW, dict(pr["par"]))
    ad = pa.AdvectionDiffusion(KW, scheme=scheme, library=lib)
    ad.discretize(g, data)
    return ad, data


# ---- 2. time stepping ---------------------------------------------------------------------------------------------
def stepping(lib, kind, precond):
    g = grid_of(kind)
    pr = problem(g)
    ad, data = discretized(lib, g, pr)
    c, info = ad.advance(g, data, pr["c0"], 5, pr["acc"], source=pr["src"], precond=precond)
    A, b = host_system(g, data[pa.DISCRETIZATION_MATRICES][KW], pr)
    ref = host_steps(A, b, pr["acc"], pr["c0"], pr["src"], 5)
    err = np.abs(c - ref).max()
    st = ad.context(g).stats()
    print(f"5 steps on {kind} ({g.num_cells} cells, {precond}): max error {err:.2e}, "
          f"{st['advdiff_iterations']} iterations, {st['advdiff_precond_fallbacks']} fallbacks")
    assert info["steps_done"] == 5 and info["converged"]
    assert err <= 1e-10


def device_vectors_and_foreign_flux(lib, to_device, to_host, n=4):
    """Every vector a device address, the flux the resident one of ANOTHER handle: same bits as the host-array path."""
    from tests._upwind_cases import flow_problem

    g = tets(n)
    fdata, fbv = flow_problem(g, np.random.default_rng(11))
    flow = pa.Mpfa("flow", library=lib)
    flow.discretize(g, fdata)
    p, _ = flow.solve(g, fdata, rtol=1e-13)
    flow.darcy_flux(g, fdata, p, resident=True)
    fctx = flow.context(g)
    pr = problem(g)
    pr["par"]["darcy_flux"] = pa.ResidentFlux(fctx)
    pr["par"]["flux_scale"] = 2.5
    ad, data = discretized(lib, g, pr)
    ctx = ad.context(g)
    assert ctx is not fctx
    c_host, info = ad.advance(g, data, pr["c0"], 5, pr["acc"], source=pr["src"])
    assert info["steps_done"] == 5
    d_bv, k1 = to_device(pr["bv"])
    d_acc, k2 = to_device(pr["acc"])
    d_src, k3 = to_device(pr["src"])
    d_c, k4 = to_device(pr["c0"].copy())
    ctx.advdiff_assemble(d_bv, None, 2.5, accumulation=d_acc, source=d_src, device=True,
                         q_device_ptr=fctx.resident_flux_ptr())
    _, dinfo = ctx.advdiff_advance(d_c, 5, device=True)
    assert dinfo["steps_done"] == 5
    assert np.array_equal(to_host(k4), c_host)
    q = fctx.resident_flux()
    A, b = host_system(g, data[pa.DISCRETIZATION_MATRICES][KW], pr, q=q, w=2.5)
    ref = host_steps(A, b, pr["acc"], pr["c0"], pr["src"], 5)
    assert np.abs(c_host - ref).max() <= 1e-10
    del k1, k2, k3


# ---- 3. Peclet regimes --------------------------------------------------------------------------------------------
def peclet(lib, pe, n=6):
    """Cell Peclet number |v| h / D with h = 1 / n and |v| of the constant velocity; D scales the tensor."""
    g = tets(n)
    vel = np.array([0.6, -0.3, 0.45])
    D = float(np.linalg.norm(vel)) / n / pe
    pr = problem(g, diffusivity=D)
    acc = np.asarray(g.cell_volumes) / 0.5  # a long step: at small Peclet numbers the system is the elliptic one
    ad, data = discretized(lib, g, pr)
    c, info = ad.advance(g, data, pr["c0"], 2, acc, source=pr["src"])  # the default call
    st = ad.context(g).stats()
    A, b = host_system(g, data[pa.DISCRETIZATION_MATRICES][KW], pr)
    ref = host_steps(A, b, acc, pr["c0"], pr["src"], 2)
    err = np.abs(c - ref).max()
    its_amg, fb = st["advdiff_iterations"], st["advdiff_precond_fallbacks"]
    print(f"Peclet {pe}: error {err:.2e}, AMG {its_amg} iterations over 2 steps, {fb} fallbacks")
    assert info["steps_done"] == 2 and info["converged"] and err <= 1e-10
    if pe <= 5:
        assert fb == 0
    if pe <= 0.05:
        cj, _ = ad.advance(g, data, pr["c0"], 2, acc, source=pr["src"], precond="jacobi")
        its_j = ad.context(g).stats()["advdiff_iterations"]
        print(f"Peclet {pe}: Jacobi {its_j} iterations over 2 steps")
        assert np.abs(cj - ref).max() <= 1e-10
        assert its_amg < its_j


def fallback_path(lib, n=4):
    """An AMG-preconditioned solve that cannot finish (one iteration allowed): the step is restored from the kept state,
    handed to Jacobi-GMRES and counted; the handle is left as it was, so the next call gives the bits of a fresh one."""
    g = tets(n)
    pr = problem(g)
    ad, data = discretized(lib, g, pr)
    ref, _ = ad.advance(g, data, pr["c0"], 2, pr["acc"], source=pr["src"])
    ctx = ad.context(g)
    assert ctx.stats()["advdiff_precond_fallbacks"] == 0
    c, info = ad.advance(g, data, pr["c0"], 2, pr["acc"], source=pr["src"], maxit=1, raise_on_fail=False)
    st = ctx.stats()
    assert info["steps_done"] == 0 and not info["converged"]  # (one Jacobi-GMRES iteration does not get there either)
    assert st["advdiff_precond_fallbacks"] == 1 and st["advdiff_gmres_retries"] == 0
    assert np.all(np.isfinite(c))
    import pytest

    with pytest.raises(pa.PorefvError) as e:
        ad.advance(g, data, pr["c0"], 1, pr["acc"], source=pr["src"], maxit=1)
    assert e.value.status == 6
    again, info = ad.advance(g, data, pr["c0"], 2, pr["acc"], source=pr["src"])
    assert info["steps_done"] == 2 and ctx.stats()["advdiff_precond_fallbacks"] == 0
    assert again.tobytes() == ref.tobytes()


# ---- 4. conservation ----------------------------------------------------------------------------------------------
def conservation(lib, n=4):
    g = tets(n)
    div = sps.csr_matrix(g.cell_faces).T.tocsr()
    pr = problem(g)
    ad, data = discretized(lib, g, pr)
    c = pr["c0"]
    for _ in range(3):
        new, info = ad.advance(g, data, c, 1, pr["acc"], source=pr["src"], rtol=1e-14)
        lhs = div @ ad.total_flux(g, data, new)
        rhs = pr["src"] - pr["acc"] * (new - c)
        err = np.abs(lhs - rhs).max() / np.abs(pr["acc"] * new).max()
        print(f"local balance: {err:.2e}")
        assert err <= 1e-11
        c = new
    # closed boundary, zero Neumann data, no source: the total amount stays
    pr = problem(g, closed=True)
    ad, data = discretized(lib, g, pr)
    total = [np.sum(pr["acc"] * pr["c0"])]
    c = pr["c0"]
    for _ in range(5):
        c, _ = ad.advance(g, data, c, 1, pr["acc"], rtol=1e-14)
        total.append(np.sum(pr["acc"] * c))
    drift = np.abs(np.array(total) - total[0]).max() / np.abs(pr["acc"] * pr["c0"]).max()
    print(f"closed domain: drift of the total {drift:.2e}")
    assert drift <= 1e-11


# ---- 5. update_flux -------------------------------------------------------------------------------------------------
def update_flux(lib, n=4):
    g = tets(n)
    pr = problem(g)
    ad, data = discretized(lib, g, pr)
    ad.solve(g, data, accumulation=pr["acc"], c_old=pr["c0"], source=pr["src"])
    ctx = ad.context(g)
    before = ctx.stats()
    q2 = -1.7 * pr["q"]
    data[pa.PARAMETERS][KW]["darcy_flux"] = q2
    ad.update_flux(g, data, accumulation=pr["acc"], c_old=pr["c0"], source=pr["src"])
    after = ctx.stats()
    for k in ("topology_ms", "symbolic_ms", "node_ms", "face_ms", "discretize_ms", "upwind_ms"):
        assert after[k] == before[k], k  # (no phase of a discretization ran)
    A1, b1 = ctx.matrix(_lib.MAT_ADVDIFF_SYSTEM), ctx.rhs()
    x1, i1 = ctx.solve(precond="amg")
    assert ctx.stats()["amg_maps_reused"] == 1  # the aggregate maps of the first setup were kept
    pr2 = problem(g)
    pr2["par"]["darcy_flux"] = q2
    ad2, data2 = discretized(lib, g, pr2)
    ad2._assemble(g, data2, pr["acc"], pr["c0"], pr["src"])
    ctx2 = ad2.context(g)
    same_csr(A1, ctx2.matrix(_lib.MAT_ADVDIFF_SYSTEM), "S after update_flux")
    assert b1.tobytes() == ctx2.rhs().tobytes()


# ---- 6. limits ------------------------------------------------------------------------------------------------------
def limits(lib, n=3):
    g = tets(n)
    pr = problem(g)
    # no diffusion: the system is Upwind's on the shared entries
    pr0 = problem(g, diffusivity=0.0)
    neu = np.asarray(pr["bc"].is_neu, bool)
    pr["bv"][neu] = 0.0  # (a Neumann value is a flux of the diffusion term too: none here)
    pr0["par"]["bc_values"] = pr["bv"]
    ad, data = discretized(lib, g, pr0, scheme="tpfa")
    A, b = ad.assemble_matrix_rhs(g, data)
    up = pa.Upwind(KW, library=lib)
    udata = pa.initialize_data({}, KW, {"darcy_flux": pr["q"], "bc": pr["bc"], "bc_values": pr["bv"]})
    up.discretize(g, udata)
    AU, bU = up.assemble_matrix_rhs(g, udata)
    assert abs(sps.csr_matrix(A) - sps.csr_matrix(AU)).max() <= 1e-14 * abs(AU).max()
    assert np.abs(b + bU).max() <= 1e-14 * np.abs(bU).max()
    # no flux: diag(acc) + A_D, bitwise
    pr["par"]["darcy_flux"] = np.zeros(g.num_faces)
    ad, data = discretized(lib, g, pr)
    ad._assemble(g, data, pr["acc"])
    ctx = ad.context(g)
    S = ctx.matrix(_lib.MAT_ADVDIFF_SYSTEM)
    A_D, _ = ad.diffusion.assemble_matrix_rhs(g, data)
    ref = sps.csr_matrix(A_D).copy()
    ref.sort_indices()
    S = sps.csr_matrix(S)
    assert np.array_equal(S.indptr, ref.indptr) and np.array_equal(S.indices, ref.indices)
    dpos = np.flatnonzero(S.indices == np.repeat(np.arange(g.num_cells), np.diff(S.indptr)))
    expect = ref.data.copy()
    expect[dpos] += pr["acc"]
    assert np.array_equal(S.data, expect)


# ---- 7. determinism, 8. isolation -----------------------------------------------------------------------------------
def _run(lib, n):
    g = tets(n)
    pr = problem(g)
    ad, data = discretized(lib, g, pr)
    A, b = ad.assemble_matrix_rhs(g, data)
    c, _ = ad.advance(g, data, pr["c0"], 3, pr["acc"], source=pr["src"])
    return [A.indptr, A.indices, A.data, b, c, ad.total_flux(g, data, c)]


def deterministic(lib, n=4):
    for x, y in zip(_run(lib, n), _run(lib, n)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def nothing_else_moves(lib, n=4):
    """Upwind matrices, the flow system and a flow solve on the SAME handle, before and after an advection-diffusion
    assembly and step on it."""
    g = tets(n)
    pr = problem(g)

    def others(mp, data):
        up = pa.Upwind(KW, library=lib, flow=mp)
        up.discretize(g, data)
        md = data[pa.DISCRETIZATION_MATRICES][KW]
        AU, bU = up.assemble_matrix_rhs(g, data)
        A, b = mp.assemble_matrix_rhs(g, data)
        x, info = mp.solve(g, data, rtol=1e-12, precond="amg")
        return [md[k] for k in ("transport", "rhs_dir", "rhs_neu")] + [AU, A], [bU, b, x], info["iterations"]

    data = pa.initialize_data({}, KW, dict(pr["par"]))
    mp = pa.Mpfa(KW, library=lib)
    mp.discretize(g, data)
    m0, v0, it0 = others(mp, data)
    ad = pa.AdvectionDiffusion(KW, diffusion=mp, library=lib)
    assert ad.context(g) is mp.context(g)
    ad.assemble_matrix_rhs(g, data)
    ad.advance(g, data, pr["c0"], 2, pr["acc"], source=pr["src"])
    m1, v1, it1 = others(mp, data)
    for a, b in zip(m0, m1):
        same_csr(a, sps.csr_matrix(b))
    for a, b in zip(v0, v1):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert it0 == it1


# ---- 9. errors ------------------------------------------------------------------------------------------------------
def errors(lib):
    import pytest

    g = geo(pa.CartGrid([4, 3], [4.0, 3.0]))
    bf = g.get_all_boundary_faces()
    pr = problem(g)
    # a Robin face
    par = dict(pr["par"], bc=pa.BoundaryCondition(g, bf, ["rob"] * bf.size))
    ad = pa.AdvectionDiffusion(KW, library=lib)
    data = pa.initialize_data({}, KW, par)
    ad.discretize(g, data)
    with pytest.raises(pa.PorefvError) as e:
        ad.assemble_matrix_rhs(g, data)
    assert e.value.status == 5
    # two components
    with pytest.raises(ValueError):
        pa.AdvectionDiffusion(KW, library=lib).discretize(g, pa.initialize_data({}, KW, dict(pr["par"], num_components=2)))
    # a periodic grid
    gp = geo(pa.CartGrid([3, 3], [1.0, 1.0]))
    gp.periodic_face_map = np.vstack([np.flatnonzero(np.isclose(gp.face_centers[0], 0.0)),
                                      np.flatnonzero(np.isclose(gp.face_centers[0], 1.0))])
    with pytest.raises(pa.PorefvError) as e:
        pa.AdvectionDiffusion(KW, library=lib).discretize(gp, pa.initialize_data({}, KW, problem(gp)["par"]))
    assert e.value.status == 5
    # a stale system: a flow assembly in between, then advance
    ad, data = discretized(lib, g, pr)
    ad.assemble_matrix_rhs(g, data)
    ad.diffusion.assemble_matrix_rhs(g, data)
    with pytest.raises(pa.PorefvError) as e:
        ad.context(g).advdiff_advance(pr["c0"], 1)
    assert e.value.status == 4
    # ... and a new discretization in between
    ad.assemble_matrix_rhs(g, data)
    ad.diffusion.discretize(g, data)
    with pytest.raises(pa.PorefvError):
        ad.context(g).advdiff_advance(pr["c0"], 1)
    with pytest.raises(pa.PorefvError):
        ad.context(g).advdiff_assemble(None, pr["q"])  # (the kept boundary values went with the discretization)
    # an inflow face that is neither Dirichlet nor Neumann
    raw = pa.bc_to_raw(pr["bc"])
    inflow = [f for f in bf if (pr["q"][f] >= 0) != (sps.find(sps.csc_matrix(g.cell_faces)[f])[2][0] > 0)]
    raw["is_dir"][inflow[0]] = raw["is_neu"][inflow[0]] = False
    ad = pa.AdvectionDiffusion(KW, scheme="tpfa", library=lib)
    data = pa.initialize_data({}, KW, dict(pr["par"], bc=_Bc(raw)))
    ad.discretize(g, data)
    with pytest.raises(ValueError, match="negative axis 1 index: -1"):
        ad.assemble_matrix_rhs(g, data)
    # a flux of the wrong length, a flux scale that is not positive
    ad, data = discretized(lib, g, pr)
    data[pa.PARAMETERS][KW]["darcy_flux"] = pr["q"][:-1]
    with pytest.raises(ValueError):
        ad.assemble_matrix_rhs(g, data)
    data[pa.PARAMETERS][KW].update(darcy_flux=pr["q"], flux_scale=-1.0)
    with pytest.raises(ValueError):
        ad.assemble_matrix_rhs(g, data)
