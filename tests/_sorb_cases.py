"""Cases of the sorbing transport step (pfv_transport_advance_sorb, ``Upwind.advance_sorbing_components``), shared by the
emulation suite (test_sorb_emulation.py) and the GPU suite (test_gpu_sorb.py): each takes the library to run on.

Judges (they never touch the library), on ``A`` and ``b_ref`` restated in scipy from ``g.cell_faces`` and ``q``
(_saturation_cases.scipy_system with the linear flux function): (J3) on an acyclic flux the cell-by-cell recursion in
flow order, one ``scipy.optimize.brentq`` per cell on ``[0, R / (acc + d)]`` with ``rtol = 8.9e-16``; (J1) a damped global
Newton solve with spsolve that keeps its iterates positive and stops at ``max|dc| <= 1e-14``.  ``judges_agree`` holds one
against the other.  J1 is not used where a Freundlich exponent below 1 starts from ``c = 0`` (its Jacobian is infinite
there).

The measured figure of ``exact`` (max|c - c_J3| over its ten (grid, isotherm) pairs, three steps from c0 = 0):
    host emulation (g++ -O2)   1.11e-15  (Langmuir on tets(3); Freundlich 0.5 on tets(4), smallest root 9.4e-9: 6.7e-16)
    gfx950 (MI355X)            1.11e-15  (the same pair)
and EXACT_BOUND is ten times the larger one.  The two judges differ by up to 1.3e-14 on these inputs themselves."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.optimize as spo
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import porepy_amd as pa
from tests import _upwind_cases as UP
from tests._multi_cases import components
from tests._saturation_cases import cfl_accumulation, core_problem, discretized, inflow_values, scipy_system
from tests._sweep_cases import VEL, edges, env, flow_order
from tests._upwind_cases import KW, data_for, geo, line_grid, tets

EXACT_MEASURED_EMULATION = 1.11e-15
EXACT_MEASURED_DEVICE = 1.11e-15
EXACT_BOUND = 10 * max(EXACT_MEASURED_EMULATION, EXACT_MEASURED_DEVICE)

ISOTHERMS = {
    "freundlich-0.5": pa.FreundlichIsotherm(1.0, 0.5),
    "freundlich-0.7": pa.FreundlichIsotherm(0.8, 0.7),
    "freundlich-1.5": pa.FreundlichIsotherm(1.0, 1.5),
    "langmuir": pa.LangmuirIsotherm(2.0, 3.0),
    "linear": pa.LinearIsotherm(1.0),
}
NONLINEAR = ["freundlich-0.5", "freundlich-0.7", "freundlich-1.5", "langmuir"]
FIVE = ["freundlich-0.5", "linear", "langmuir", "freundlich-1.5", "freundlich-0.7"]


def slope(iso, c):
    """S'(c), restated here (c > 0 where a Freundlich exponent is below 1)"""
    c = np.asarray(c, dtype=float)
    if isinstance(iso, pa.LinearIsotherm):
        return np.full_like(c, iso.kd)
    if isinstance(iso, pa.FreundlichIsotherm):
        return iso.kf * iso.n * c ** (iso.n - 1.0)
    return iso.q_max * iso.b / (1.0 + iso.b * c) ** 2


# ---- the judges -----------------------------------------------------------------------------------------------------
def recursion_steps(g, q, bv, acc, cap, iso, c0, n, source=None):
    """(J3) one component on an acyclic flux: cell by cell in flow order, every cell one brentq"""
    A, bref = scipy_system(g, q, bv, "linear")
    A = sps.csr_matrix(A)
    d = A.diagonal()
    order = flow_order(g.num_cells, *edges(g, q))
    assert order["core_cells"] == 0
    src = np.zeros(g.num_cells) if source is None else source
    c = c0.copy()
    for _ in range(n):
        rhs = acc * c + cap * iso(c) - bref + src
        new = np.zeros(g.num_cells)
        for i in order["order"]:
            cols, vals = A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]
            R = rhs[i] - sum(v * new[j] for j, v in zip(cols, vals) if j != i)  # (the upstream cells are known)
            D = acc[i] + d[i]
            if R <= 0.0:
                assert R > -1e-13 * (abs(rhs[i]) + 1e-300), (i, R)
                continue
            gi = lambda x: D * x + cap[i] * float(iso(x)) - R  # noqa: E731
            new[i] = R / D if gi(R / D) == 0.0 else spo.brentq(gi, 0.0, R / D, xtol=1e-300, rtol=8.9e-16, maxiter=4000)
        c = new
    return c


def newton_steps(g, q, bv, acc, cap, iso, c0, n, source=None):
    """(J1) one component on any flux: damped global Newton, the iterates kept positive"""
    A, bref = scipy_system(g, q, bv, "linear")
    A = sps.csr_matrix(A)
    src = np.zeros(g.num_cells) if source is None else source
    c = c0.copy()
    for _ in range(n):
        old, s_old = c, iso(c)

        def F(x):
            return acc * (x - old) + cap * (iso(x) - s_old) + A @ x + bref - src

        x = np.maximum(old, 1e-3)  # (a start inside c > 0)
        r = F(x)
        for _ in range(200):
            dx = spla.spsolve((sps.diags(acc + cap * slope(iso, x)) + A).tocsc(), -r)
            t = 1.0
            while True:
                xn = x + t * dx
                if xn.min() > 0.0:
                    rn = F(xn)
                    if np.linalg.norm(rn) <= (1 - 1e-4 * t) * np.linalg.norm(r) or np.abs(t * dx).max() <= 1e-12:
                        break
                assert t > 1e-12, "the judge's Newton solve cannot stay positive"
                t *= 0.5
            x, r = xn, rn
            if np.abs(t * dx).max() <= 1e-14:
                break
        else:
            raise AssertionError("the judge's Newton solve did not converge")
        c = x
    return c


def line_recursion(iso, acc, cap, c0, n, inflow=1.0, source=None):
    """the line with q = 1: cell i is one scalar equation given cell i - 1"""
    nc = c0.size
    src = np.zeros(nc) if source is None else source
    c = c0.copy()
    for _ in range(n):
        new = np.empty(nc)
        up = inflow
        for i in range(nc):
            R = acc[i] * c[i] + cap[i] * float(iso(c[i])) + up + src[i]
            gi = lambda x: (acc[i] + 1.0) * x + cap[i] * float(iso(x)) - R  # noqa: E731
            new[i] = spo.brentq(gi, 0.0, R / (acc[i] + 1.0), xtol=1e-300, rtol=8.9e-16, maxiter=4000) if cap[i] > 0 else R / (acc[i] + 1.0)
            up = new[i]
        c = new
    return c


def tets_problem(n, cfl=5.0):
    g = tets(n)
    q = pa.Upwind(KW).darcy_flux(g, VEL)
    acc = cfl_accumulation(g, q, cfl)
    return g, q, inflow_values(g, 1.0), acc, 0.5 * acc


def line_problem():
    g = line_grid(16, 2.0)
    bv = np.zeros(g.num_faces)
    bv[0] = 1.0
    bc = pa.BoundaryCondition(g, g.get_all_boundary_faces(), ["dir", "dir"])
    return g, np.ones(g.num_faces), bv, bc, np.full(16, 0.5), np.full(16, 0.5)


# ---- 0. the judges against each other (no library) ----------------------------------------------------------------------
def judges_agree():
    g, q, bv, acc, cap = tets_problem(3)
    c0 = np.full(g.num_cells, 0.05)
    for name in ("freundlich-0.7", "langmuir", "freundlich-1.5"):
        j1 = newton_steps(g, q, bv, acc, cap, ISOTHERMS[name], c0, 3)
        j3 = recursion_steps(g, q, bv, acc, cap, ISOTHERMS[name], c0, 3)
        err = np.abs(j1 - j3).max()
        print(f"tets(3), {name}: max|c_J1 - c_J3| = {err:.2e}")
        assert err <= 2e-14  # (J1 stops at max|dc| <= 1e-14, J3 at a relative 8.9e-16)
        assert j3.max() - j3.min() > 0.05  # (a front is there)


# ---- 1. exact on an acyclic flux ------------------------------------------------------------------------------------------
_j3 = {}


def exact(lib, n, name):
    g, q, bv, acc, cap = tets_problem(n)
    iso, c0 = ISOTHERMS[name], np.zeros(g.num_cells)
    if (n, name) not in _j3:  # (the reference is computed once, and shared by the two suites)
        _j3[n, name] = recursion_steps(g, q, bv, acc, cap, iso, c0, 3)
    ref = _j3[n, name]
    up, data = discretized(lib, g, q, bv)
    c, info = up.advance_sorbing_components(g, data, c0[None], 3, acc, iso, capacity=cap)
    st = up.context(g).stats()
    err = np.abs(c[0] - ref).max()
    print(f"tets({n}), {name}: max|c - c_J3| = {err:.2e} after 3 steps at CFL 5, smallest root {ref[ref > 0].min():.1e}, "
          f"relative residual {info['rel_residual'][0]:.2e}, {st['sweep_levels']} levels, {st['sweep_launches']} launches")
    assert info["steps_done"] == 3 and info["converged"] and info["iterations"] == [1]
    assert st["sweep_core_cells"] == 0 and st["transport_sorb_steps"] == 3 and st["transport_sorb_core_iterations"] == 0
    assert st["transport_sorb_components"] == 1
    assert info["rel_residual"][0] <= 1e-12
    assert ref.max() - ref.min() > 0.05 and c.min() >= 0.0
    assert err <= EXACT_BOUND
    return err


# ---- 2. the line against its recursion ----------------------------------------------------------------------------------
def line_case(lib, name):
    g, q, bv, bc, acc, cap = line_problem()
    iso, c0 = ISOTHERMS[name], np.zeros(16)
    ref = line_recursion(iso, acc, cap, c0, 5)
    up, data = discretized(lib, g, q, bv, bc)
    c, info = up.advance_sorbing_components(g, data, c0[None], 5, acc, iso, capacity=cap)
    st = up.context(g).stats()
    plain, _ = up.advance_sorbing_components(g, data, c0[None], 5, acc, iso)
    err = np.abs(c[0] - ref).max()
    print(f"line, {name}: max|c - c_recursion| = {err:.2e}; against no capacity: {c[0, 0] - plain[0, 0]:.2e} in cell 0, "
          f"{c[0, 15] - plain[0, 15]:.2e} in cell 15")
    assert info["steps_done"] == 5 and st["sweep_levels"] == 16 and st["sweep_core_cells"] == 0
    assert err <= 1e-13
    assert np.abs(plain[0] - line_recursion(iso, acc, 0.0 * cap, c0, 5)).max() <= 1e-13
    assert abs(c[0, 0] - plain[0, 0]) > 1e-3 and abs(c[0, 15] - plain[0, 15]) > 1e-3  # (the term acts)


# ---- 3. linear is the linear step, bit for bit -------------------------------------------------------------------------------
def linear_is_the_linear_step(lib, n=4, k=3):
    g = tets(n)
    q, bc, acc, bv, c0, source = components(g, k)
    assert c0.min() >= 0 and bv.min() >= 0 and source.min() >= 0
    cap = acc * np.random.default_rng(11).random((k, g.num_cells))
    up, data = discretized(lib, g, q, bv[0], bc)
    c, info = up.advance_sorbing_components(g, data, c0, 3, acc, pa.LinearIsotherm(1.0), capacity=cap, bc_values=bv,
                                            source=source)
    st = up.context(g).stats()
    lin, ldata = discretized(lib, g, q, bv[0], bc)
    want, linfo = lin.advance_components(g, ldata, c0, 3, acc + cap, bc_values=bv, source=source, precond="sweep",
                                         rtol=1e-13)
    lst = lin.context(g).stats()
    assert info["steps_done"] == 3 and linfo["steps_done"] == 3 and lst["transport_multi_direct_steps"] == 3
    print(f"Kd = 1 against advance_components(acc + cap): largest difference {np.abs(c - want).max():.1e}")
    assert c.tobytes() == want.tobytes()
    assert st["sweep_launches"] == lst["sweep_launches"] > 0 and st["sweep_levels"] == lst["sweep_levels"]
    assert np.abs(info["sorbed"] - c).max() == 0.0
    assert np.abs(c - c0).max() > 1e-3


# ---- 4. components do not see each other ------------------------------------------------------------------------------------
def independent(lib, k, solo):
    """k components cycling FIVE, each with its own boundary values, capacity and state; the components in ``solo``
    against the k = 1 call of each alone"""
    g, q, bv0, acc0, _ = tets_problem(4)
    nc = g.num_cells
    rng = np.random.default_rng(17)
    iso = [ISOTHERMS[FIVE[a % 5]] for a in range(k)]
    bv = np.array([(0.25 + 0.75 * rng.random()) * bv0 for _ in range(k)])
    acc = np.array([(1.0 + 0.1 * (a % 7)) * acc0 for a in range(k)])
    cap = acc * rng.random((k, nc))
    c0 = 0.3 * rng.random((k, nc)) * (rng.random((k, nc)) < 0.7)  # (some cells start from 0)
    up, data = discretized(lib, g, q, bv0)
    c, info = up.advance_sorbing_components(g, data, c0, 3, acc, iso, capacity=cap, bc_values=bv)
    assert info["steps_done"] == 3 and up.context(g).stats()["transport_sorb_components"] == k
    for a in solo:
        one, i1 = up.advance_sorbing_components(g, data, c0[a:a + 1], 3, acc[a:a + 1], iso[a], capacity=cap[a:a + 1],
                                                bc_values=bv[a:a + 1])
        assert i1["steps_done"] == 3
        assert one[0].tobytes() == c[a].tobytes(), (k, a)
        assert i1["sorbed"][0].tobytes() == info["sorbed"][a].tobytes(), (k, a)
        assert np.abs(one[0] - c0[a]).max() > 1e-3


# ---- 5. a cyclic core converges ---------------------------------------------------------------------------------------------
def core_converges(lib, which):
    g, q, cfl, _, n_core = core_problem(which)
    nc = g.num_cells
    bv, acc = inflow_values(g, 1.0), cfl_accumulation(g, q, cfl)
    cap, c0 = 0.5 * acc, np.full((2, nc), 0.05)
    iso = [ISOTHERMS["freundlich-0.7"], ISOTHERMS["langmuir"]]
    ref = np.array([newton_steps(g, q, bv, acc, cap, one, c0[0], 3) for one in iso])
    up, data = discretized(lib, g, q, bv)
    c, info = up.advance_sorbing_components(g, data, c0, 3, acc, iso, capacity=cap, rtol=1e-12)
    st = up.context(g).stats()
    err = np.abs(c - ref).max(axis=1)
    print(f"{which}: max|c - c_J1| = {['%.2e' % e for e in err]} after 3 steps at CFL {cfl}, core of "
          f"{st['sweep_core_cells']} cells, {st['transport_sorb_core_iterations']} core iterations in all, "
          f"{info['iterations']} in the last step, relative residuals {['%.1e' % r for r in info['rel_residual']]}")
    assert info["steps_done"] == 3 and info["converged"] and max(info["rel_residual"]) <= 1e-12
    assert st["sweep_core_cells"] == n_core and st["transport_sorb_steps"] == 3
    for a in range(2):
        assert st["transport_sorb_core_iterations"] >= info["iterations"][a] > 0
    assert err.max() <= 1e-10
    assert np.abs(ref - 0.05).max() > 1e-2
    # two iterations are not enough: the call says so and hands the state back untouched
    c2, i2 = up.advance_sorbing_components(g, data, c0, 3, acc, iso, capacity=cap, maxit=2, raise_on_fail=False)
    assert i2["steps_done"] == 0 and not i2["converged"] and i2["iterations"] == [2, 2]
    assert c2.tobytes() == c0.tobytes()
    with pytest.raises(pa.PorefvError) as e:
        up.advance_sorbing_components(g, data, c0, 3, acc, iso, capacity=cap, maxit=2)
    assert e.value.status == 6 and "did not settle in 2 iterations" in e.value.message
    assert e.value.state.tobytes() == c0.tobytes() and e.value.info["steps_done"] == 0


# ---- 6. deterministic, and the two launch forms agree ------------------------------------------------------------------------
def deterministic_and_merged(lib, n=6):
    g, q, bv, acc, cap = tets_problem(n)
    iso = [ISOTHERMS[m] for m in ("freundlich-0.5", "freundlich-0.7", "langmuir", "linear")]
    c0 = np.zeros((4, g.num_cells))
    runs = []
    for environment in ({}, {}, {"PFV_SWEEP_MERGE": 0}):
        with env(**environment):
            up, data = discretized(lib, g, q, bv)
            c, info = up.advance_sorbing_components(g, data, c0, 3, acc, iso, capacity=cap)
            st = up.context(g).stats()
        assert info["steps_done"] == 3
        runs.append((c, st["sweep_launches"], st["sweep_levels"], info["sorbed"]))
    print("launches per sweep (merged, merged, one per level):", [r[1] for r in runs])
    for r in runs[1:]:
        assert r[0].tobytes() == runs[0][0].tobytes() and r[3].tobytes() == runs[0][3].tobytes()
    assert runs[2][1] == runs[2][2] and runs[0][1] < runs[2][1]
    g, q, cfl, _, _ = core_problem("cyclic12")
    bv, acc = inflow_values(g, 1.0), cfl_accumulation(g, q, cfl)
    both = []
    for _ in range(2):
        up, data = discretized(lib, g, q, bv)
        both.append(up.advance_sorbing_components(g, data, np.full((4, g.num_cells), 0.05), 2, acc, iso,
                                                  capacity=0.5 * acc)[0])
    assert both[0].tobytes() == both[1].tobytes()


# ---- 7. mass ----------------------------------------------------------------------------------------------------------------
def mass(lib, n=4, rtol=1e-12):
    g, q, bv, acc, cap = tets_problem(n)
    nc = g.num_cells
    rng = np.random.default_rng(21)
    names = NONLINEAR + ["linear"]
    k = len(names)
    c0 = 0.2 * rng.random((k, nc))
    source = np.zeros((k, nc))
    source[:, nc // 2] = 0.05 * acc[0]
    A, bref = scipy_system(g, q, bv, "linear")
    up, data = discretized(lib, g, q, bv)
    c, info = up.advance_sorbing_components(g, data, c0, 1, acc, [ISOTHERMS[m] for m in names], capacity=cap,
                                            source=source, rtol=rtol)
    assert info["steps_done"] == 1
    for a, name in enumerate(names):
        iso = ISOTHERMS[name]
        rhs = acc * c0[a] + cap * iso(c0[a]) - bref + source[a]
        defect = abs(np.sum(acc * (c[a] - c0[a]) + cap * (iso(c[a]) - iso(c0[a])) + (A @ c[a] + bref) - source[a]))
        bound = np.sqrt(nc) * rtol * np.linalg.norm(rhs)
        ulps = np.abs(info["sorbed"][a] - iso(c[a])) / np.spacing(iso(c[a]))
        print(f"{name}: |sum of the balance| = {defect:.2e} (bound {bound:.2e}); sorbed against the numpy curve: "
              f"{ulps.max():.1f} ulp")
        assert defect <= bound
        assert ulps.max() <= 4.0
        assert np.abs(c[a] - c0[a]).max() > 1e-3


# ---- 8. no non-negative root -------------------------------------------------------------------------------------------------
def no_root(lib):
    g, q, bv, bc, acc, cap = line_problem()
    iso, c0 = ISOTHERMS["freundlich-0.7"], np.zeros((1, 16))
    source = np.zeros((1, 16))
    source[0, 5] = -1.0
    up, data = discretized(lib, g, q, bv, bc)
    with pytest.raises(ValueError, match=r"step 0 leaves c >= 0: no root in cell 5, component 0$") as e:
        up.advance_sorbing_components(g, data, c0, 3, acc, iso, capacity=cap, source=source)
    assert e.value.state.tobytes() == c0.tobytes() and e.value.info["steps_done"] == 0
    assert up.context(g).stats()["transport_sorb_steps"] == 0
    # the same source in the second of two components
    two = np.vstack([0.0 * source, source])
    with pytest.raises(ValueError, match=r"step 0 leaves c >= 0: no root in cell 5, component 1$") as e:
        up.advance_sorbing_components(g, data, np.zeros((2, 16)), 3, acc, [ISOTHERMS["langmuir"], iso], capacity=cap,
                                      source=two)
    assert e.value.state.tobytes() == np.zeros((2, 16)).tobytes() and e.value.info["steps_done"] == 0
    # the handle serves a correct call afterwards
    c, info = up.advance_sorbing_components(g, data, c0, 5, acc, iso, capacity=cap)
    assert info["steps_done"] == 5
    assert np.abs(c[0] - line_recursion(iso, acc, cap, c0[0], 5)).max() <= 1e-13


# ---- 9. errors ------------------------------------------------------------------------------------------------------------
class _RawIsotherm(pa.LinearIsotherm):
    """a (kind, parameters) pair no class would produce, for the checks of the C entry point through ``Upwind``"""

    def __init__(self, kind, p0, p1):
        self.kind, self._p = kind, (p0, p1)

    def params(self):
        return np.array(self._p, dtype=float)


def errors(lib):
    g = geo(pa.CartGrid([4, 3], [4.0, 3.0]))
    nc, nf = g.num_cells, g.num_faces
    bf = g.get_all_boundary_faces()
    q = pa.Upwind(KW).darcy_flux(g, [1.0, 0.5, 0.0])
    cfd = sps.csc_matrix(g.cell_faces)
    inflow = np.array([f for f in bf if (q[f] >= 0) != (sps.find(cfd[f])[2][0] > 0)])
    outflow = np.setdiff1d(bf, inflow)
    k = 2
    bv1, acc1 = inflow_values(g, 1.0), cfl_accumulation(g, q, 2.0)
    bv, acc, cap, c0 = np.array([bv1, 0.5 * bv1]), np.array([acc1, 2.0 * acc1]), np.array([0.5 * acc1, acc1]), np.full((k, nc), 0.1)
    iso = [ISOTHERMS["freundlich-0.7"], ISOTHERMS["langmuir"]]
    A, bref = scipy_system(g, q, bv1, "linear")
    ref = spla.spsolve((sps.diags(acc1) + A).tocsc(), acc1 * c0[0] - bref)

    def changed(x, idx, v):
        y = np.array(x, dtype=float, copy=True)
        y[idx] = v
        return y

    def refused(up, data, status, text, **change):
        """the call is refused with that status and text; afterwards the handle serves a correct advance_components"""
        a = dict(c0=c0, acc=acc, iso=iso, capacity=cap, bc_values=bv)
        a.update(change)
        c0_, acc_, iso_ = a.pop("c0"), a.pop("acc"), a.pop("iso")
        with pytest.raises(ValueError if status == 4 else pa.PorefvError, match=re.escape(text)) as e:
            up.advance_sorbing_components(g, data, c0_, 1, acc_, iso_, **a)
        if status != 4:
            assert e.value.status == status
        good = data_for(q, None, bv1)
        up.discretize(g, good)
        c, info = up.advance_components(g, good, c0[:1], 1, acc1, precond="sweep")
        assert info["steps_done"] == 1 and np.abs(c[0] - ref).max() <= 1e-12

    up = pa.Upwind(KW, library=lib)
    data = data_for(q, None, bv1)
    # call order
    with pytest.raises((ValueError, pa.PorefvError)):
        up.advance_sorbing_components(g, data, c0, 1, acc, iso, capacity=cap, bc_values=bv)
    d2 = data_for(q, None, bv1, k=2)
    up.discretize(g, d2)
    refused(up, d2, 4, "num_components = 1")
    up.discretize(g, data)
    ctx = up.context(g)
    # k = 0 and k = 65, at both levels
    dp, ip, ptr = pa._lib._dp, pa._lib._ip, pa._lib._ptr
    for kk in (0, 65):
        with pytest.raises(ValueError, match=rf"1 \.\. 64, not {kk} "):
            up.advance_sorbing_components(g, data, np.zeros((kk, nc)), 1, np.ones(nc), iso[0])
        m = max(kk, 1)
        st = ctx.lib.pfv_transport_advance_sorb(ctx._h, None, kk, ptr(np.zeros(m, dtype=np.int32), ip), ptr(np.ones(2 * m), dp),
                                                ptr(np.zeros(m * nf), dp), ptr(np.ones(m * nc), dp), None, None, 1, 1e-12,
                                                10, ptr(np.zeros(m * nc), dp), None, None, None)
        assert st == 4 and f"k = {kk}" in ctx.lib.pfv_last_error(ctx._h).decode()
    # the isotherms, each with the first offender
    with pytest.raises(ValueError, match="isotherms must be one isotherm or a list of 2, not 3"):
        up.advance_sorbing_components(g, data, c0, 1, acc, iso + iso[:1], capacity=cap, bc_values=bv)
    with pytest.raises(ValueError, match=r"isotherms\[1\] must be a LinearIsotherm"):
        up.advance_sorbing_components(g, data, c0, 1, acc, [iso[0], "linear"], capacity=cap, bc_values=bv)
    for bad, text in ((_RawIsotherm(7, 1.0, 1.0), "isotherm of component 1: unknown isotherm kind 7"),
                      (_RawIsotherm(-1, 1.0, 1.0), "isotherm of component 1: unknown isotherm kind -1"),
                      (pa.LinearIsotherm(-1.0), "component 1: linear isotherm parameter Kd (index 0) is negative"),
                      (pa.LinearIsotherm(np.nan), "component 1: linear isotherm parameter Kd (index 0) is not finite"),
                      (pa.FreundlichIsotherm(-0.5, 0.7), "component 1: Freundlich parameter Kf (index 0) is negative"),
                      (pa.FreundlichIsotherm(1.0, 0.0), "component 1: Freundlich parameter n (index 1) must be positive"),
                      (pa.FreundlichIsotherm(1.0, -2.0), "component 1: Freundlich parameter n (index 1) must be positive"),
                      (pa.FreundlichIsotherm(np.inf, 0.7), "component 1: Freundlich parameter Kf (index 0) is not finite"),
                      (pa.FreundlichIsotherm(1.0, np.nan), "component 1: Freundlich parameter n (index 1) is not finite"),
                      (pa.LangmuirIsotherm(-2.0, 3.0), "component 1: Langmuir parameter q_max (index 0) is negative"),
                      (pa.LangmuirIsotherm(2.0, -3.0), "component 1: Langmuir parameter b (index 1) is negative"),
                      (pa.LangmuirIsotherm(2.0, np.inf), "component 1: Langmuir parameter b (index 1) is not finite")):
        refused(up, data, 4, text, iso=[iso[0], bad])
    refused(up, data, 4, "isotherm of component 0: Freundlich parameter n (index 1) must be positive",
            iso=[pa.FreundlichIsotherm(1.0, 0.0), pa.LangmuirIsotherm(-1.0, 1.0)])  # (the first offender)
    # the arrays, each with the lowest offender
    refused(up, data, 4, "accumulation must be positive: cell 5, component 1",
            acc=changed(changed(acc, (1, 5), 0.0), (0, 9), -1.0))
    refused(up, data, 4, "accumulation must be positive: cell 7, component 0", acc=changed(acc, (0, 7), np.nan))
    refused(up, data, 4, "capacity must not be negative: cell 3, component 1",
            capacity=changed(changed(cap, (1, 3), -1e-3), (0, 8), -1.0))
    refused(up, data, 4, "capacity must not be negative: cell 6, component 0", capacity=changed(cap, (0, 6), np.nan))
    refused(up, data, 4, "c must be non-negative and finite: cell 4, component 1",
            c0=changed(changed(c0, (1, 4), -1e-12), (0, 6), np.inf))
    refused(up, data, 4, "c must be non-negative and finite: cell 2, component 0", c0=changed(c0, (0, 2), np.nan))
    b2 = changed(bv, (slice(None), outflow), -7.0)  # values on outflow faces are not read
    got, info = up.advance_sorbing_components(g, data, c0, 1, acc, iso, capacity=cap, bc_values=b2)
    assert info["steps_done"] == 1
    f_lo, f_hi = sorted(inflow[[1, 2]])
    refused(up, data, 4, f"Dirichlet inflow value must be non-negative and finite: face {f_lo}, component 1",
            bc_values=changed(changed(bv, (1, f_lo), -0.5), (0, f_hi), np.inf))
    refused(up, data, 4, f"Dirichlet inflow value must be non-negative and finite: face {f_hi}, component 0",
            bc_values=changed(bv, (0, f_hi), np.nan))
    # a Neumann face: any finite value is a flux, a non-finite one is refused
    kinds = np.array(["dir"] * bf.size, dtype=object)
    kinds[np.isin(bf, inflow[:1])] = "neu"
    neu = pa.BoundaryCondition(g, bf, list(kinds))
    ndata = data_for(q, neu, bv1)
    up.discretize(g, ndata)
    got, info = up.advance_sorbing_components(g, ndata, c0, 1, acc, iso, capacity=cap,
                                              bc_values=changed(bv, (slice(None), inflow[0]), -0.01))
    assert info["steps_done"] == 1
    refused(up, ndata, 4, f"Neumann value is not finite on face {inflow[0]}, component 1",
            bc_values=changed(bv, (1, inflow[0]), np.inf))
    # the inflow-face rule: a Robin face that has outflow in the discretization, inflow in the flux of the call
    kinds = np.array(["dir"] * bf.size, dtype=object)
    kinds[np.isin(bf, outflow[:2])] = "rob"
    rob = pa.BoundaryCondition(g, bf, list(kinds))
    up.discretize(g, data_for(q, rob, bv1))
    refused(up, data_for(-q, rob, bv1), 4, f"face {outflow[:2].min()}")
    # shapes, named
    up.discretize(g, data)
    with pytest.raises(ValueError, match=rf"c0 must have shape \(k, {nc}\)"):
        up.advance_sorbing_components(g, data, c0[0], 1, acc, iso[0])
    with pytest.raises(ValueError, match=rf"capacity must have shape \({nc},\) or \(2, {nc}\)"):
        up.advance_sorbing_components(g, data, c0, 1, acc, iso, capacity=cap[:, :-1])
    with pytest.raises(ValueError, match=r"accumulation must have shape"):
        up.advance_sorbing_components(g, data, c0, 1, acc[:1, :3], iso)
    with pytest.raises(ValueError, match=r"bc_values must have shape"):
        up.advance_sorbing_components(g, data, c0, 1, acc, iso, bc_values=np.zeros((3, nf)))
    with pytest.raises(ValueError, match=r"source must have shape"):
        up.advance_sorbing_components(g, data, c0, 1, acc, iso, source=np.zeros((2, nc + 1)))
    with pytest.raises(ValueError, match="accumulation is required"):
        up.advance_sorbing_components(g, data, c0, 1, None, iso)
    with pytest.raises(ValueError, match=r"isotherm_kinds must have shape \(2,\)"):
        ctx.transport_advance_sorb(c0, 1, acc, bv, [0], np.ones((2, 2)))
    # periodic grids, conditions per sub-face
    gp = geo(pa.CartGrid([3, 3], [1.0, 1.0]))
    gp.periodic_face_map = np.vstack([np.flatnonzero(np.isclose(gp.face_centers[0], 0.0)),
                                      np.flatnonzero(np.isclose(gp.face_centers[0], 1.0))])
    with pytest.raises(pa.PorefvError) as e:
        pa.Upwind(KW, library=lib).advance_sorbing_components(
            gp, data_for(np.ones(gp.num_faces), None, np.zeros(gp.num_faces)), np.zeros((2, 9)), 1, np.ones(9), iso)
    assert e.value.status == 5
    fdata, _ = UP.flow_problem(g, np.random.default_rng(23))
    mp = pa.Mpfa("flow", library=lib)
    mp.discretize(g, fdata)
    ups = pa.Upwind(KW, library=lib, flow=mp)
    ups.discretize(g, data)
    fctx = mp.context(g)
    fctx.set_subface_bc(np.ones(fctx.nsf, dtype=np.uint8))  # (Dirichlet on every sub-face; only the switch matters here)
    with pytest.raises(pa.PorefvError) as e:
        ups.advance_sorbing_components(g, data, c0, 1, acc, iso, capacity=cap, bc_values=bv)
    assert e.value.status == 5 and "sub-face" in e.value.message
    fctx.set_subface_bc(None)
    got, info = ups.advance_sorbing_components(g, data, c0, 1, acc, iso, capacity=cap, bc_values=bv)
    assert info["steps_done"] == 1


# ---- 10. lifetime ---------------------------------------------------------------------------------------------------------
def lifetime(lib, n=4):
    g, q, bv, acc, cap = tets_problem(n)
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    iso = [ISOTHERMS["freundlich-0.7"], ISOTHERMS["linear"]]
    c0 = np.full((2, g.num_cells), 0.1)
    up, data = discretized(lib, g, q, bv, bc)
    ctx = up.context(g)
    # no assembly is needed, and none is left behind
    c, info = up.advance_sorbing_components(g, data, c0, 2, acc, iso, capacity=cap)
    assert info["steps_done"] == 2 and ctx.stats()["sweep_order_ms"] > 0
    assert ctx.active_size() == 0
    with pytest.raises(RuntimeError):
        ctx.solve()
    with pytest.raises(pa.PorefvError):
        ctx.transport_advance(np.zeros(g.num_cells), 1)
    # the same flux again: the order is kept, the result is the same; n_steps = 0 hands c0 and S(c0) back
    c2, _ = up.advance_sorbing_components(g, data, c0, 2, acc, iso, capacity=cap)
    assert ctx.stats()["sweep_order_ms"] == 0 and c2.tobytes() == c.tobytes()
    c3, i3 = up.advance_sorbing_components(g, data, c0, 0, acc, iso, capacity=cap)
    assert i3["steps_done"] == 0 and c3.tobytes() == c0.tobytes()
    assert np.abs(i3["sorbed"][0] - iso[0](c0[0])).max() <= 4 * np.spacing(iso[0](0.1))
    assert i3["sorbed"][1].tobytes() == c0[1].tobytes()
    # other edges: the order is rebuilt
    first = ctx.sweep_info()
    d2 = data_for(-q, bc, bv)
    up.discretize(g, d2)
    up.advance_sorbing_components(g, d2, c0, 1, acc, iso, capacity=cap)
    assert ctx.stats()["sweep_order_ms"] > 0
    assert not np.array_equal(first["level"], ctx.sweep_info()["level"])
    # a selected preconditioner stays selected: the C call below selects nothing itself
    jac, jdata = discretized(lib, g, q, bv, bc)
    c1, i1 = jac.advance(g, jdata, c0[0], 1, acc, method="gmres")  # selects "jacobi"
    jac.advance_sorbing_components(g, jdata, c0, 1, acc, iso, capacity=cap)
    jctx = jac.context(g)
    jac._assemble(g, jdata, acc, None, None)
    x, done, last = c0[0].copy(), C.c_int32(0), pa._lib.SolveInfo()
    st = jctx.lib.pfv_transport_advance(jctx._h, 1, pa._lib.SOLVE_GMRES, 1e-12, 20000, pa._lib._ptr(x, pa._lib._dp),
                                        C.byref(done), C.byref(last))
    assert st == 0 and done.value == 1 and last.iterations == i1["iterations"] > 1
    assert x.tobytes() == c1.tobytes() and jctx.stats()["sweep_direct_steps"] == 0
    # the C call with NULL for everything optional
    dp, ip, ptr = pa._lib._dp, pa._lib._ip, pa._lib._ptr
    cc = c0.copy()
    kinds, par = np.array([1, 0], dtype=np.int32), np.array([[0.8, 0.7], [1.0, 0.0]])
    st = ctx.lib.pfv_transport_advance_sorb(ctx._h, None, 2, ptr(kinds, ip), ptr(par, dp),
                                            ptr(np.ascontiguousarray(np.broadcast_to(bv, (2, g.num_faces))), dp),
                                            ptr(np.ascontiguousarray(np.broadcast_to(acc, (2, g.num_cells))), dp), None,
                                            None, 1, 1e-12, 10, ptr(cc, dp), None, C.byref(done), None)
    assert st == 0 and done.value == 1 and ctx.stats()["transport_sorb_steps"] == 1


def flow_system_is_untouched(lib, n=3):
    """Upwind(flow=mpfa) shares the handle: after the sorbing call the flow system assembles and solves to the bits of a
    handle that never saw it (the model: _saturation_cases.flow_system_is_untouched)."""
    def flow(with_transport):
        g = tets(n)
        fdata, _ = UP.flow_problem(g, np.random.default_rng(23))
        mp = pa.Mpfa("flow", library=lib)
        mp.discretize(g, fdata)
        p, _ = mp.solve(g, fdata, rtol=1e-12)
        if with_transport:
            mp.darcy_flux(g, fdata, p, resident=True)
            up = pa.Upwind(KW, library=lib, flow=mp)
            assert up.context(g) is mp.context(g)
            tdata = pa.initialize_data({}, KW, {"bc_values": inflow_values(g, 1.0)})
            up.discretize(g, tdata)
            qd = np.abs(mp.context(g).resident_flux())
            acc = np.full(g.num_cells, 4 * qd.max())
            c, info = up.advance_sorbing_components(g, tdata, np.full((2, g.num_cells), 0.1), 2, acc,
                                                    [ISOTHERMS["freundlich-0.5"], ISOTHERMS["langmuir"]],
                                                    capacity=0.5 * acc, maxit=2000)
            assert info["steps_done"] == 2 and c.max() > 0.1 + 1e-6
        A, b = mp.assemble_matrix_rhs(g, fdata)
        x, info = mp.solve(g, fdata, rtol=1e-12)
        return p, A, b, x, info["iterations"], mp.context(g).matrix(pa._lib.MAT_FLUX)

    p1, A1, b1, x1, it1, F1 = flow(True)
    p2, A2, b2, x2, it2, F2 = flow(False)
    UP.same_csr(A1, A2, "A")
    UP.same_csr(F1, F2, "flux")
    assert p1.tobytes() == p2.tobytes() and np.asarray(b1).tobytes() == np.asarray(b2).tobytes()
    assert x1.tobytes() == x2.tobytes() and it1 == it2
