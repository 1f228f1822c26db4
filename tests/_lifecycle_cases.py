"""One handle driven through every call that makes a system the active one, with a solve after each: nothing derived
from the values of an earlier system (hierarchy, renumbered copy, SpMV window, extracted blocks) may survive.  Shared by
the emulation suite (test_lifecycle_emulation.py) and the GPU suite (test_gpu_lifecycle.py): each case takes the library.

Judges: the true residual in numpy on the matrix and right-hand side the library exports (for user systems: the arrays
that were passed in), and a fresh handle that performs only the last discretize / assemble / solve."""
import ctypes as C
import hashlib

import numpy as np
import scipy.sparse as sps

import porepy_amd as pa
from porepy_amd import _lib
from porepy_amd.device_csr import DeviceCsr
from porepy_amd.distributed import permute_cells
from porepy_amd.params import bc_flags
from tests._sweep_cases import env

N = 20            # 20 x 20 cells: above PFV_REORDER_MIN_CELLS = 256, the renumbered copy is in play
RTOL = 1e-10
RES_FACTOR = 10.0  # true residual <= RES_FACTOR * RTOL: the gap between the recurrence residual and the true one
WINDOW_ENV = {"PFV_SPMV_WINDOW_MIN_NNZ": 500}  # (read per call) below the nnz of every system of the walk
GRID_KINDS = ("flow", "adflux", "transport", "advdiff", "mech")
APPLIES = {"jacobi": GRID_KINDS + ("user",), "amg": ("flow", "adflux", "advdiff", "mech", "user"),
           "sweep": ("transport", "advdiff"), "block": ("user",)}
WALKS = [("jacobi", False), ("jacobi", True), ("amg", False), ("amg", True), ("sweep", True), ("block", True)]

_PROBLEM = {}
_FRESH = {}


def problem(lib):
    """The grid and every input of the walk, made once per library."""
    key = id(lib)
    if key in _PROBLEM:
        return _PROBLEM[key]
    g = pa.CartGrid([N, N], [1.0, 1.0])
    g.compute_geometry()
    raw = pa.grid_to_raw(g)
    rng = np.random.default_rng(11)
    nc, nf = g.num_cells, g.num_faces
    bf = g.get_all_boundary_faces()

    def perm(k):
        K = np.zeros((3, 3, nc))
        K[0, 0], K[1, 1], K[2, 2] = k, 2.0 * k, 1.0
        K[0, 1] = K[1, 0] = 0.2 * k
        return K

    P = {"g": g, "nc": nc, "nf": nf, "K1": perm(1.0 + rng.random(nc)), "K2": perm(np.exp(2.0 * rng.random(nc))),
         "flags": bc_flags(pa.BoundaryCondition(g, bf, ["dir"] * bf.size))}
    bv = np.zeros(nf)
    bv[bf] = 1.0 + g.face_centers[0, bf] + 0.5 * g.face_centers[1, bf] ** 2
    P["bv"] = bv
    # the grid's own numbering must not follow the curve: else shuffle it (fixed seed)
    ctx = _lib.Context(0, lib)
    ctx.set_grid(raw)
    _flow(P, "K1")(ctx)
    p, _ = ctx.solve(rtol=1e-12)
    if ctx.stats()["solve_renumbered"] != 1:
        order = np.random.default_rng(5).permutation(nc)
        raw = permute_cells(raw, order)
        for k in ("K1", "K2"):
            P[k] = np.ascontiguousarray(P[k][:, :, order])
        ctx.set_grid(raw)
        _flow(P, "K1")(ctx)
        p, _ = ctx.solve(rtol=1e-12)
        assert ctx.stats()["solve_renumbered"] == 1
    P["raw"] = raw
    P["q"] = ctx.face_flux(p, bv)
    ctx.close()
    P["p_ad"] = 1.0 + rng.random(nc)
    P["dk"] = 0.1 * P["K2"]
    vol = np.asarray(raw["cell_volumes"], dtype=float)
    P["acc"] = vol * (0.5 + rng.random(nc)) / 0.05
    P["c0"] = rng.random(nc)
    P["bvc"] = np.where(np.isin(np.arange(nf), bf), rng.random(nf), 0.0)
    nd = 2
    P["stiff"] = pa.FourthOrderTensor(1.0 + rng.random(nc), 1.0 + rng.random(nc)).values
    P["bcm"] = pa.BoundaryConditionVectorial(g, bf, ["dir"] * bf.size)
    P["bvm"] = np.where(np.tile(np.isin(np.arange(nf), bf), nd), rng.random(nd * nf), 0.0)
    P["src_m"] = rng.random(nd * nc)
    for name, n, seed in (("U1", 300, 1), ("U2", 260, 2), ("U3", 300, 3)):
        P[name] = _user_matrix(n, seed)
    _PROBLEM[key] = P
    return P


def _user_matrix(n, seed):
    """Tridiagonal, diagonally dominant, plus one far column per row; not symmetric."""
    rng = np.random.default_rng(seed)
    far = (np.arange(n) + n // 2 + 7) % n
    A = sps.diags([-1.0 - rng.random(n - 1), 4.0 + rng.random(n), -0.5 - rng.random(n - 1)], [-1, 0, 1]).tocsr()
    A = (A + sps.csr_matrix((0.3 * rng.random(n), (np.arange(n), far)), shape=(n, n))).tocsr()
    A.sort_indices()
    return A, rng.random(n)


# ---- the steps: each returns a function of the handle that ends with the system active ----------------------------
def _flow(P, K, again=False, set_k=False):
    def run(ctx):
        if not again:
            if set_k:
                ctx.set_permeability(P[K])
            else:
                ctx.set_params(P[K], P["flags"])
            ctx.discretize()
        ctx.assemble(P["bv"])
    return run


def _adflux(P):
    return lambda ctx: ctx.ad_flux_system(P["p_ad"], dk_dp=P["dk"], bc_values=P["bv"])


def _transport(P, sign):
    def run(ctx):
        ctx.upwind_discretize(sign * P["q"])
        ctx.upwind_assemble(P["bvc"], accumulation=P["acc"], c_old=P["c0"])
    return run


def _advdiff(P, w, refresh=False):
    def run(ctx):
        ctx.advdiff_assemble(bc_values=None if refresh else P["bvc"], q=P["q"], flux_scale=w, accumulation=P["acc"],
                             c_old=P["c0"])
    return run


def _mech(P, again=False):
    def run(ctx):
        if not again:
            ctx.mpsa_set_params(P["stiff"], P["raw"]["cell_volumes"], P["bcm"].is_dir, P["bcm"].is_neu)
            ctx.mpsa_discretize()
        ctx.mpsa_assemble(P["bvm"], P["src_m"])
    return run


def _user(P, name, csr=False):
    def run(ctx):
        A, b = P[name]
        if csr:
            DeviceCsr.from_scipy(A, ctx).as_system(b)
        else:
            ctx.set_system(A, b)
    return run


def _seq(*fs):
    def run(ctx):
        for f in fs:
            f(ctx)
    return run


def steps(P):
    """(name, kind, what the walked handle does, what a fresh handle with the grid does).  Every revisit reuses the value
    buffer of an earlier system."""
    f1, f2 = _flow(P, "K1"), _flow(P, "K2")
    return [
        ("flow K1", "flow", f1, f1),
        ("flow K2 (re-discretize, re-assemble)", "flow", _flow(P, "K2", set_k=True), f2),
        ("ad_flux_system", "adflux", _adflux(P), _seq(f2, _adflux(P))),
        ("flow after ad_flux_system", "flow", _flow(P, "K2", again=True), f2),
        ("transport q", "transport", _transport(P, 1.0), _transport(P, 1.0)),
        ("transport -q", "transport", _transport(P, -1.0), _transport(P, -1.0)),
        ("flow after transport", "flow", _flow(P, "K2", again=True), f2),
        ("advdiff w=1", "advdiff", _advdiff(P, 1.0), _seq(f2, _advdiff(P, 1.0))),
        ("advdiff refresh w=2", "advdiff", _advdiff(P, 2.0, refresh=True), _seq(f2, _advdiff(P, 2.0))),
        ("flow after advdiff", "flow", _flow(P, "K2", again=True), f2),
        ("mechanics", "mech", _mech(P), _mech(P)),
        ("set_system U1 after mechanics", "user", _user(P, "U1"), _user(P, "U1")),
        ("mechanics after set_system", "mech", _mech(P, again=True), _mech(P)),
        ("set_system U3 (the pattern of U1, other values)", "user", _user(P, "U3"), _user(P, "U3")),
        ("csr_set_system U2 (another size)", "user", _user(P, "U2", csr=True), _user(P, "U2", csr=True)),
        ("set_system U1 again", "user", _user(P, "U1"), _user(P, "U1")),
    ]


WHICH = {"flow": _lib.MAT_SYSTEM, "adflux": _lib.MAT_SYSTEM, "transport": _lib.MAT_TRANSPORT_SYSTEM,
         "advdiff": _lib.MAT_ADVDIFF_SYSTEM, "mech": _lib.MAT_MECH_SYSTEM}


def _solve(ctx, precond, n_user):
    if precond == "block" and getattr(ctx, "_block_n", None) != n_user:  # (kept while the size stays: its blocks are a cache)
        ctx.set_block_preconditioner(np.array([0, n_user // 3, n_user], dtype=np.int64))
        ctx._block_n = n_user
    x, info = ctx.solve(method="bicgstab", rtol=RTOL, precond=precond)
    return np.array(x), info, ctx.stats()


def _setup_ran(ctx, before, after):
    """Did the solve that left the statistics `after` set a hierarchy up?  amg_setup_launches on the HIP library; the
    emulation build launches nothing, there a setup shows as a newly measured amg_setup_ms."""
    if ctx.lib.pfv_is_device_build():
        return after["amg_setup_launches"] > 0
    return after["amg_setup_ms"] != before["amg_setup_ms"]


def _system(ctx, P, name, kind):
    if kind == "user":
        return P[name.split()[1]]  # ("set_system U1 ...")
    return sps.csr_matrix(ctx.matrix(WHICH[kind])), np.array(ctx.rhs())


def _fresh(lib, P, name, kind, precond, windows, run):
    key = (id(lib), name, precond, windows)
    if key not in _FRESH:
        ctx = _lib.Context(0, lib)
        if kind != "user":
            ctx.set_grid(P["raw"])
        run(ctx)
        A, _ = _system(ctx, P, name, kind)
        x, info, _ = _solve(ctx, precond, A.shape[0])
        ctx.close()
        _FRESH[key] = (x.tobytes(), info["iterations"])
    return _FRESH[key]


def walk(lib, precond, windows, bits_except=()):
    """The scripted walk with `precond` wherever it applies (Jacobi elsewhere).  `bits_except`: names of steps compared by
    residual alone.  Returns the trace, one line per solve."""
    P = problem(lib)
    trace = []
    with env(**(WINDOW_ENV if windows else {})):
        ctx = _lib.Context(0, lib)
        ctx.set_grid(P["raw"])
        for name, kind, run, fresh in steps(P):
            pc = precond if kind in APPLIES[precond] else "jacobi"
            run(ctx)
            A, b = _system(ctx, P, name, kind)
            st0 = ctx.stats()
            x, info, st = _solve(ctx, pc, A.shape[0])
            res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
            line = (f"trace {precond}{'+win' if windows else ''} | {name} [{pc}]: it {info['iterations']} renumbered "
                    f"{st['solve_renumbered']} setup {int(_setup_ran(ctx, st0, st))} maps_reused {st['amg_maps_reused']} "
                    f"levels {st['amg_levels']} x {hashlib.sha256(x.tobytes()).hexdigest()[:16]}")
            print(line, f"| true residual / rtol {res / RTOL:.2f}")
            trace.append(line)
            assert info["converged"], name
            assert res <= RES_FACTOR * RTOL, (name, res)
            assert st["solve_renumbered"] == (0 if kind == "user" else 1), name
            if pc == "amg":
                assert _setup_ran(ctx, st0, st), name  # the values changed: the hierarchy is set up again
            x2, info2, st2 = _solve(ctx, pc, A.shape[0])  # nothing changed: nothing is set up again
            assert info2["iterations"] == info["iterations"], name
            assert st2["solve_renumbered"] == st["solve_renumbered"]
            if pc == "amg":
                assert not _setup_ran(ctx, st, st2), name
            else:
                assert x2.tobytes() == x.tobytes(), name
                xf, itf = _fresh(lib, P, name, kind, pc, windows, fresh)
                assert itf == info["iterations"], (name, itf, info["iterations"])
                if name not in bits_except:
                    assert xf == x.tobytes(), name
        ctx.close()
    return trace


# ---- the advance calls: a step that fails without a NaN -------------------------------------------------------------
def advance_not_converged(lib, which):
    """maxit = 1: the first step ends with PFV_ERR_NOT_CONVERGED.  The call reports it with the solver's message, leaves
    steps_done at the completed steps, hands back the state of the failed step, and leaves the handle's vector mode and
    preconditioner as they were (a host-array AMG solve follows)."""
    P = problem(lib)
    nc = P["nc"]
    ctx = _lib.Context(0, lib)
    ctx.set_grid(P["raw"])
    if which == "transport":
        assemble = _transport(P, 1.0)
        assemble(ctx)
        call, mat = ctx.lib.pfv_transport_advance, _lib.MAT_TRANSPORT_SYSTEM
    else:
        assemble = _advdiff(P, 1.0)
        _seq(_flow(P, "K2"), assemble)(ctx)
        call, mat = ctx.lib.pfv_advdiff_advance, _lib.MAT_ADVDIFF_SYSTEM
    A = sps.csr_matrix(ctx.matrix(mat))
    ctx._select_precond("amg")  # (transport: replaced by Jacobi inside the call; advdiff: used, then the Jacobi fallback)
    c = P["c0"].copy()
    done, info = C.c_int32(-1), _lib.SolveInfo()
    st = call(ctx._h, 3, _lib.SOLVE_GMRES, 1e-13, 1, _lib._ptr(c, _lib._dp), C.byref(done), C.byref(info))
    assert st == 6, st
    assert done.value == 0
    assert ctx.lib.pfv_last_error(ctx._h).decode() == "Krylov solver did not reach the requested tolerance"
    assert info.iterations == 1 and not info.converged and np.isfinite(info.rel_residual)
    assert np.all(np.isfinite(c)) and not np.array_equal(c, P["c0"])
    # the state handed back is the iterate of the failed solve, not the input: it is closer to the step's solution
    b = np.array(ctx.rhs())  # (the right-hand side of the step from c0)
    assert np.linalg.norm(b - A @ c) < np.linalg.norm(b - A @ P["c0"])
    stats = ctx.stats()
    if which == "advdiff":
        assert stats["advdiff_precond_fallbacks"] == 1 and stats["advdiff_iterations"] == 2
    else:
        assert stats["transport_iterations"] == 1 and stats["transport_gmres_retries"] == 0
    # assembled again (so that a hierarchy has to be set up), then no set_preconditioner and no vector mode before the
    # solve: host arrays, and the AMG that was selected before the call
    assemble(ctx)
    stats = ctx.stats()
    x = np.empty(nc)
    i2 = _lib.SolveInfo()
    st = ctx.lib.pfv_solve(ctx._h, _lib.SOLVE_BICGSTAB, RTOL, 1000, 0, None, _lib._ptr(x, _lib._dp), C.byref(i2))
    assert st == 0 and i2.converged
    assert _setup_ran(ctx, stats, ctx.stats())
    assert np.linalg.norm(b - A @ x) <= RES_FACTOR * RTOL * np.linalg.norm(b)
    ctx.close()
    return f"trace advance {which}: rel_residual {info.rel_residual!r} c {hashlib.sha256(c.tobytes()).hexdigest()[:16]}"


# ---- vectors on the device: every output equals its host-array counterpart -------------------------------------------
def device_outputs(lib, to_device, to_host):
    P = problem(lib)
    nc, nf = P["nc"], P["nf"]
    ctx = _lib.Context(0, lib)
    ctx.set_grid(P["raw"])
    _flow(P, "K2")(ctx)
    keep = []

    def dev(a):
        ptr, t = to_device(np.ascontiguousarray(a, dtype=np.float64))
        keep.append(t)
        return ptr, t

    def same(host, t, what):
        ctx.sync()
        assert np.asarray(host).tobytes() == to_host(t).tobytes(), what

    x, _ = ctx.solve(rtol=RTOL)
    px, tx = dev(np.zeros(nc))
    ctx.solve_device(px, rtol=RTOL)
    same(x, tx, "pfv_solve")
    pp, _ = dev(x)
    pb, _ = dev(P["bv"])
    q = ctx.face_flux(x, P["bv"])
    pq, tq = dev(np.zeros(nf))
    ctx.face_flux(pp, pb, device=True, q_ptr=pq)
    same(q, tq, "pfv_mpfa_face_flux")
    pr, tr = dev(np.zeros(nf))
    ctx._dev(True)
    try:
        ctx._check(ctx.lib.pfv_resident_flux(ctx._h, None, C.cast(pr, _lib._dp)))
    finally:
        ctx._dev(False)
    same(ctx.resident_flux(), tr, "pfv_resident_flux")
    pbc, _ = dev(P["bvc"])
    pacc, _ = dev(P["acc"])
    pc0, _ = dev(P["c0"])
    ctx.upwind_discretize(q)
    bref = ctx.upwind_assemble(P["bvc"], accumulation=P["acc"], c_old=P["c0"], bound_rhs=True)
    pbr, tbr = dev(np.zeros(nc))
    ctx.upwind_assemble(pbc, accumulation=pacc, c_old=pc0, device=True, bound_rhs_ptr=pbr)
    same(bref, tbr, "bound_rhs_out of pfv_upwind_assemble")
    bref = ctx.advdiff_assemble(bc_values=P["bvc"], q=q, accumulation=P["acc"], c_old=P["c0"], bound_rhs=True)
    pba, tba = dev(np.zeros(nc))
    ctx.advdiff_assemble(bc_values=pbc, q=pq, accumulation=pacc, c_old=pc0, device=True, bound_rhs_ptr=pba)
    same(bref, tba, "bound_rhs_out of pfv_advdiff_assemble")
    flux = ctx.advdiff_face_flux(P["c0"])
    pf, tf = dev(np.zeros(nf))
    ctx.advdiff_face_flux(pc0, device=True, out_ptr=pf)
    same(flux, tf, "pfv_advdiff_face_flux")
    ctx.close()
