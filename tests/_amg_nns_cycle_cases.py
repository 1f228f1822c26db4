"""The cycle of the near-null-space AMG (csrc/amg_nns.inc) against an independent reference, shared by the emulation
suite (test_amg_nns_emulation.py) and the GPU suite (test_gpu_amg_nns.py): each case takes the library to run on.

The reference (RefNnsCycle) is written from the header comment of amg_nns.inc.  It uses the read-out of the hierarchy
(Context.amg_nns_level: A_l, P_l, agg) and the switches the case itself sets, nothing else: the inverses of the diagonal
blocks and the coarsest solve are recomputed on the host.  The library's cycle is applied alone, through
Context.amg_nns_apply_device.

Tolerance, as in _amg_cases.py and never from the library's output: the reference is evaluated in longdouble (inverses
refined by Newton steps, coarsest solve by residual refinement) and in float64 with the rows of every matrix stored in
the opposite order and plain float64 inverses.  The library sums in float64 in yet another order, so its error is of the
class of the second evaluation: it gets FACTOR = 16 times the float64-vs-longdouble difference on the case's own vectors,
and 0 < bound <= 1e-10 is asserted for every case."""
import contextlib
import os

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sps

import porepy_amd as pa
from porepy_amd import _lib
from tests import _amg_cases as AC
from tests import _amg_nns_cases as NC

LD = np.longdouble
FACTOR, HARD = AC.FACTOR, AC.HARD
DENSE_MAX = 1024  # the coarsest level is solved exactly up to this many rows (amg.inc: kAmgDenseMax)
FALLBACK_STEPS = 3  # block-Jacobi steps after the first one on a coarsest level above it
PREFIX = "PFV_AMG_NNS_"


@contextlib.contextmanager
def environment(env):
    """The PFV_AMG_NNS_* switches of `env` (short names), every other one of the family unset."""
    full = {PREFIX + k: str(v) for k, v in env.items()}
    stray = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith(PREFIX) and k not in full}
    try:
        with AC.environment(full):
            yield
    finally:
        os.environ.update(stray)


def switches(env, n0):
    """What nns_read_switches / amg_nns_setup make of the case's switches (the documented defaults and clamps)."""
    gamma = int(env["GAMMA"]) if "GAMMA" in env else (2 if n0 >= 600000 else 1)
    return {"omega": 0.01 * int(env.get("OMEGA_PCT", 70)), "alpha": 0.01 * int(env.get("ALPHA_PCT", 130)),
            "fp32": int(env.get("FP32", 1)) != 0, "gamma": max(1, min(2, gamma)),
            "gamma_levels": max(1, int(env.get("GAMMA_LEVELS", 1))), "sweeps": max(1, min(4, int(env.get("SWEEPS", 1))))}


def read_hierarchy(ctx):
    lev0 = ctx.amg_nns_level(0)
    return [lev0] + [ctx.amg_nns_level(l) for l in range(1, lev0["levels"])]


def prolongator(lev):
    """P_l as hierarchy_identities builds it: row r -> columns agg(r) k .. agg(r) k + k - 1."""
    n, bs, k, nagg = lev["n"], lev["block_size"], lev["k"], lev["aggregates"]
    row_agg = np.repeat(lev["agg"].astype(np.int64), bs)
    return sps.csr_matrix((lev["P"].ravel(), (np.repeat(np.arange(n), k), (row_agg[:, None] * k + np.arange(k)).ravel())),
                          shape=(n, nagg * k))


def diagonal_blocks(A, bs):
    """[cells][bs][bs] diagonal blocks of a CSR matrix (FP64 values as read out)."""
    row = AC.row_of_entries(A)
    on = (row // bs) == (A.indices // bs)
    D = np.zeros((A.shape[0] // bs, bs, bs))
    np.add.at(D, (row[on] // bs, row[on] % bs, A.indices[on] % bs), A.data[on])
    return D


def refined_inverses(D):
    """longdouble inverses of the blocks: numpy.linalg.inv in float64, then Newton steps X <- X (2 I - D X) until the
    update is below 1e-30 -- or, where longdouble has fewer digits than that (x87: 64 bits), until it has stopped
    shrinking at the rounding of the format, which is asserted."""
    X = np.linalg.inv(D).astype(LD)
    Dl = D.astype(LD)
    I2 = 2 * np.eye(D.shape[1], dtype=LD)
    prev = np.inf
    for _ in range(12):
        Xn = np.matmul(X, I2 - np.matmul(Dl, X))
        step = float(np.max(np.abs(Xn - X).max(axis=(1, 2)) / np.abs(Xn).max(axis=(1, 2))))
        X = Xn
        if step < 1e-30 or step >= prev:
            break
        prev = step
    assert step <= 256 * np.finfo(LD).eps, ("the block inverses of the reference did not settle", step)
    return X


def reversed_csr(M, dtype):
    M = sps.csr_matrix(M)
    M = AC.reversed_rows(M)
    return sps.csr_matrix((M.data.astype(dtype), M.indices, M.indptr), shape=M.shape)


class RefNnsCycle:
    """x = M_0 b of amg_nns.inc on read-out data.  Level l: x = omega D^-1 b, sweeps - 1 block-Jacobi steps,
    b_c = P^T (b - A x), the coarse cycle (a second one on b_c - A_c x_c, added, when gamma == 2, l < gamma_levels and
    l + 2 < levels), x += alpha P x_c, sweeps block-Jacobi steps.  Coarsest level: the exact solve up to DENSE_MAX rows,
    above it omega D^-1 b and three block-Jacobi steps.  The products read FP32-rounded values when the switch is on; the
    block inverses and the coarsest solve come from the FP64 values."""

    def __init__(self, H, sw, dtype=LD, reverse=False):
        self.sw, self.dtype, self.nlev = sw, dtype, len(H)
        self.A, self.P, self.Pt, self.Dinv, self.bs = [], [], [], [], []
        exact = dtype is LD
        for l, lev in enumerate(H):
            M = sps.csr_matrix(lev["A"])
            data = M.data.astype(np.float32).astype(np.float64) if sw["fp32"] else M.data
            Mr = sps.csr_matrix((data, M.indices, M.indptr), shape=M.shape)
            self.A.append(reversed_csr(Mr, dtype) if reverse else Mr.astype(dtype))
            D = diagonal_blocks(M, lev["block_size"])
            self.Dinv.append(refined_inverses(D) if exact else np.linalg.inv(D))
            self.bs.append(lev["block_size"])
            if l + 1 < self.nlev:
                Pm = prolongator(lev)
                Pt = sps.csr_matrix(Pm.T)
                self.P.append(reversed_csr(Pm, dtype) if reverse else Pm.astype(dtype))
                self.Pt.append(reversed_csr(Pt, dtype) if reverse else Pt.astype(dtype))
        self.omega, self.alpha = dtype(sw["omega"]), dtype(sw["alpha"])
        last = sps.csr_matrix(H[-1]["A"])
        self.direct = None
        if last.shape[0] <= DENSE_MAX:
            dense = last.toarray()
            if exact:
                self.direct = (sla.lu_factor(dense), last.astype(LD))
            else:
                self.direct = np.linalg.inv(dense[::-1])[:, ::-1] if reverse else np.linalg.inv(dense)
        self.second_visits = 0
        self.fallbacks = 0

    def dinv(self, l, v):
        bs = self.bs[l]
        return np.einsum("cij,cj->ci", self.Dinv[l], v.reshape(-1, bs)).reshape(-1)

    def smooth(self, l, x, b):
        return x + self.omega * self.dinv(l, b - self.A[l] @ x)

    def coarsest(self, l, b):
        if self.direct is None:
            self.fallbacks += 1
            x = self.omega * self.dinv(l, b)
            for _ in range(FALLBACK_STEPS):
                x = self.smooth(l, x, b)
            return x
        if self.dtype is not LD:
            return self.direct @ b
        lu, Al = self.direct
        x = sla.lu_solve(lu, b.astype(np.float64)).astype(LD)
        prev = np.inf
        for _ in range(12):  # until the correction has stopped shrinking (the longdouble rounding of the residual)
            dx = sla.lu_solve(lu, (b - Al @ x).astype(np.float64)).astype(LD)
            x = x + dx
            step = float(np.abs(dx).max())
            if step == 0.0 or step >= prev:
                break
            prev = step
        return x

    def cycle(self, l, b):
        if l + 1 == self.nlev:
            return self.coarsest(l, b)
        sw = self.sw
        x = self.omega * self.dinv(l, b)
        for _ in range(sw["sweeps"] - 1):
            x = self.smooth(l, x, b)
        bc = self.Pt[l] @ (b - self.A[l] @ x)
        xc = self.cycle(l + 1, bc)
        if sw["gamma"] == 2 and l < sw["gamma_levels"] and l + 2 < self.nlev:
            self.second_visits += 1
            xc = xc + self.cycle(l + 1, bc - self.A[l + 1] @ xc)
        x = x + self.alpha * (self.P[l] @ xc)
        for _ in range(sw["sweeps"]):
            x = self.smooth(l, x, b)
        return x

    def __call__(self, R):
        return np.array([self.cycle(0, np.asarray(r, dtype=self.dtype)) for r in np.atleast_2d(R)])


def apply_cycle(ctx, lib, R):
    """pfv_amg_nns_apply_device on the rows of R.  Emulation build: "device" pointers are host pointers."""
    R = np.ascontiguousarray(np.atleast_2d(R), dtype=np.float64)
    if lib.pfv_is_device_build():
        import torch

        r = torch.from_numpy(R).cuda()
        z = torch.zeros_like(r)
        torch.cuda.synchronize()
        for i in range(R.shape[0]):
            ctx.amg_nns_apply_device(r[i].data_ptr(), z[i].data_ptr())
        ctx.sync()
        return z.cpu().numpy()
    Z = np.zeros_like(R)
    for i in range(R.shape[0]):
        ctx.amg_nns_apply_device(R[i].ctypes.data, Z[i].ctypes.data)
    ctx.sync()
    return Z


def vectors(H, seed=0):
    """case_vectors of _amg_cases.py on the level-0 read-out (no aggregates on a hierarchy of one level)."""
    lev0 = dict(H[0], agg=H[0]["agg"] if H[0]["aggregates"] else None)
    return AC.case_vectors([lev0], seed)


def check_cycle(ctx, lib, H, sw, seed=0):
    V = vectors(H, seed)
    Z = apply_cycle(ctx, lib, V)
    ref = RefNnsCycle(H, sw, LD)
    Zref = ref(V)
    Zalt = RefNnsCycle(H, sw, np.float64, reverse=True)(V)
    base = AC.max_rel(Zalt, Zref)
    bound = FACTOR * base
    err = AC.max_rel(Z, Zref)
    print("amg_nns cycle: baseline %.3g bound %.3g error %.3g ratio %.3g" % (base, bound, err, err / bound))
    assert 0 < bound <= HARD, ("the case is ill-conditioned for the purpose", bound)
    assert err <= bound, ("cycle", err, bound)
    # linearity at rounding level, and two applies are the same bits
    a, b = 0.75, -1.5
    lin = apply_cycle(ctx, lib, a * V[0] + b * V[1])[0]
    lerr = AC.max_rel(lin, (a * Z[0].astype(LD) + b * Z[1].astype(LD))[None, :])
    assert lerr <= bound, ("linearity", lerr, bound)
    assert np.array_equal(apply_cycle(ctx, lib, V[:3]), Z[:3]), "two applies differ"
    return {"baseline": base, "bound": bound, "error": err, "ratio": err / bound, "ref": ref}


# ---------------------------------------------------------------------------------------------------------------------
# systems

def largest_aggregate_rows(lev):
    return int(np.bincount(lev["agg"]).max()) * lev["block_size"]


def widest_row_lds(lev):
    """bytes of LDS nns_galerkin asks for the widest block row of this (coarse) level: k^2 doubles and one int32 per
    block column, 16 bytes of slack (the request the 48 KiB and 150 KiB thresholds act on)"""
    k = lev["block_size"]
    cols = int(np.diff(lev["A"].indptr).max()) // k
    return 8 * cols * k * k + 4 * cols + 16


def pair_system(pairs, bs, k, seed=11):
    """Disjoint pairs of cells: the Laplacian of the pairs (x) an SPD block, plus a random positive diagonal.  One
    coarsening (every pair an aggregate), then nothing is left to match."""
    rng = np.random.default_rng(seed)
    L = sps.kron(sps.eye(pairs), np.array([[1.0, -1.0], [-1.0, 1.0]]))
    K = rng.standard_normal((bs, bs))
    K = K @ K.T + bs * np.eye(bs)
    n = 2 * pairs * bs
    A = sps.csr_matrix(sps.kron(L, K) + sps.diags(0.5 + rng.random(n)))
    return A, rng.standard_normal((n, k)), rng.standard_normal(n)


def isolated_blocks(cells, bs, k, seed=12):
    rng = np.random.default_rng(seed)
    blocks = []
    for _ in range(cells):
        K = rng.standard_normal((bs, bs))
        blocks.append(K @ K.T + bs * np.eye(bs))
    n = cells * bs
    return sps.csr_matrix(sps.block_diag(blocks)), rng.standard_normal((n, k)), rng.standard_normal(n)


def hub_system(n_cells, bs=3, k=8):
    """user_system plus a hub: cell 0 coupled to every cell by 1e-3 (11^T + I) blocks on a graph Laplacian."""
    A, B, b = NC.user_system(n_cells, bs, k, isolated=False)
    others = np.arange(1, n_cells)
    zero = np.zeros(others.size, dtype=np.int64)
    G = sps.csr_matrix((np.ones(2 * others.size), (np.concatenate([zero, others]), np.concatenate([others, zero]))),
                       shape=(n_cells, n_cells))
    Lh = sps.diags(np.asarray(G.sum(axis=1)).ravel()) - G
    A = sps.csr_matrix(A + sps.kron(Lh, 1e-3 * (np.ones((bs, bs)) + np.eye(bs))))
    return A, B, b


def rank_deficient_system():
    A, B, b = NC.user_system(400, 3, 6, isolated=False)
    B = B.copy()
    B[:, 3] = B[:, 0]
    B[:, 5] = 0.0
    return A, B, b


def clamped_mpsa(lib, g, seed=1):
    """MPSA matrix of a grid with its bottom clamped and a mild contrast, and the grid's rigid-body modes."""
    S = AC.MechSystem(lib, g, seed)
    return S.A, pa.rigid_body_modes(g), np.asarray(S.b)


# name -> (system, block size, switches, what the read-out must show: expect(H, ref))
def _levels_at_least(m):
    def expect(H, ref):
        assert len(H) >= m, len(H)
    return expect


def _second_visit(H, ref):
    assert len(H) >= 4, len(H)
    assert ref.second_visits > 0


def _second_visit_two_levels(H, ref):
    _second_visit(H, ref)
    # one apply runs cycle(0) once, cycle(1) twice: level 0 counts one second visit, level 1 two
    assert ref.second_visits >= 3 * len(vectors(H)), ref.second_visits


def _default_300(H, ref):
    assert [h["n"] for h in H] == [900, 828, 366], [h["n"] for h in H]
    assert np.bincount(H[0]["agg"]).min() == 1  # the isolated cell


def _wide_aggregates(rows):
    def expect(H, ref):
        assert largest_aggregate_rows(H[0]) > rows, largest_aggregate_rows(H[0])
    return expect


def _stalled(levels):
    def expect(H, ref):
        assert len(H) == levels and H[-1]["n"] > DENSE_MAX, (len(H), H[-1]["n"])
        assert ref.fallbacks > 0 and ref.direct is None
    return expect


def _rank_deficient(H, ref):
    Pm = prolongator(H[0])
    dropped = np.flatnonzero(np.asarray((Pm.T @ Pm).diagonal()) < 0.5)
    assert dropped.size == 2 * H[0]["aggregates"], (dropped.size, H[0]["aggregates"])  # two zero columns everywhere
    d1 = H[1]["A"].diagonal()
    assert np.all(d1[dropped] == 1.0)


def _wide_row(H, ref):
    lds = widest_row_lds(H[1])
    assert 48 * 1024 < lds < 150 * 1024, lds


def _blocks(bs, k):
    def expect(H, ref):
        assert len(H) >= 2 and H[0]["block_size"] == bs and H[0]["k"] == k and H[1]["block_size"] == k
    return expect


def _one_level(H, ref):
    assert len(H) == 1


W2 = {"GAMMA": 2, "COARSE_TARGET": 60, "SWEEPS": 2}
USER_CASES = {
    "default": (lambda: NC.user_system(300, 3, 6), 3, {}, _default_300),
    "fp32=0": (lambda: NC.user_system(300, 3, 6), 3, {"FP32": 0}, _default_300),
    "gamma=2,sweeps=2": (lambda: NC.user_system(1200, 3, 6), 3, W2, _second_visit),
    "gamma=2,sweeps=2,levels=2": (lambda: NC.user_system(1200, 3, 6), 3, dict(W2, GAMMA_LEVELS=2),
                                  _second_visit_two_levels),
    "sweeps=4": (lambda: NC.user_system(1200, 3, 6), 3, {"SWEEPS": 4}, _levels_at_least(2)),
    "omega=55,alpha=100": (lambda: NC.user_system(1200, 3, 6), 3, {"OMEGA_PCT": 55, "ALPHA_PCT": 100},
                           _levels_at_least(2)),
    "passes=6 (aggregates of 144 rows)": (lambda: NC.user_system(2000, 3, 6), 3,
                                          {"PASSES": 6, "PASSES_COARSE": 4, "COARSE_TARGET": 30}, _wide_aggregates(128)),
    "bs=8,k=8 (aggregates of 152 rows)": (lambda: NC.user_system(400, 8, 8, isolated=False), 8, {}, _wide_aggregates(64)),
    "stalled pairs (1,1)": (lambda: pair_system(1200, 1, 1), 1, {}, _stalled(2)),
    "stalled pairs (3,6)": (lambda: pair_system(400, 3, 6), 3, {}, _stalled(2)),
    "isolated blocks: one level of 1200 rows": (lambda: isolated_blocks(400, 3, 6), 3, {}, _stalled(1)),
    "rank-deficient modes on every aggregate": (rank_deficient_system, 3, {}, _rank_deficient),
    "hub: coarse row between 48 and 150 KiB": (lambda: hub_system(1500), 3, {}, _wide_row),
}
for _n, _bs, _k in ((400, 2, 3), (400, 3, 1), (400, 3, 3), (400, 5, 2), (400, 4, 8), (400, 8, 1), (700, 1, 1), (700, 1, 3)):
    USER_CASES["bs=%d,k=%d" % (_bs, _k)] = (lambda n=_n, bs=_bs, k=_k: NC.user_system(n, bs, k, isolated=False), _bs, {},
                                           _blocks(_bs, _k))
MPSA_CASES = {
    "mpsa 2-d": (lambda: NC.grid_2d(8), {}, _one_level),  # 256 rows: below the coarsening target, the exact solve alone
    "mpsa 2-d, coarsened": (lambda: NC.grid_2d(8), {"COARSE_TARGET": 60}, _blocks(2, 3)),
    "mpsa 3-d": (lambda: NC.grid_3d(4), {}, _blocks(3, 6)),
}


def build_and_check(lib, A, B, b, bs, env, expect, seed=0):
    """set_system, set_near_null_space, a solve of one iteration to build the hierarchy under the case's switches;
    read-out, identities, the path the case is for, the cycle."""
    ctx = _lib.Context(0, lib)
    with environment(env):
        ctx.set_system(A, b)
        ctx.set_near_null_space(B, bs)
        ctx.solve(method="cg", rtol=1e-10, maxit=1, raise_on_fail=False, precond="amg_nns")
        H = read_hierarchy(ctx)
        if len(H) >= 2:
            NC.hierarchy_identities(ctx)
        sw = switches(env, A.shape[0])
        out = check_cycle(ctx, lib, H, sw, seed)
        expect(H, out["ref"])
    out["H"] = H
    return out


def user_case(lib, name):
    make, bs, env, expect = USER_CASES[name]
    A, B, b = make()
    return build_and_check(lib, A, B, b, bs, env, expect)


def mpsa_case(lib, name):
    make, env, expect = MPSA_CASES[name]
    g = make()
    A, B, b = clamped_mpsa(lib, g)
    return build_and_check(lib, A, B, b, g.dim, env, expect)


def too_wide_is_refused(lib):
    """The hub at 4000 cells: its coarse block row does not fit the LDS, the setup says so, and the handle goes on."""
    A, B, b = hub_system(4000)
    ctx = _lib.Context(0, lib)
    with environment({}):
        ctx.set_system(A, b)
        ctx.set_near_null_space(B, 3)
        try:
            ctx.solve(method="cg", rtol=1e-10, maxit=1, raise_on_fail=False, precond="amg_nns")
        except _lib.PorefvError as e:
            assert e.status == 5 and "too wide for LDS" in e.message, (e.status, e.message)
        else:
            raise AssertionError("a coarse block row beyond 150 KiB of LDS was accepted")
        A2, B2, b2 = NC.user_system(300, 3, 6)
        ctx.set_system(A2, b2)
        ctx.set_near_null_space(B2, 3)
        x, info = ctx.solve(method="cg", rtol=1e-10, precond="amg_nns")
        assert info["converged"]
        assert np.linalg.norm(b2 - A2 @ x) <= 1e-9 * np.linalg.norm(b2)
        NC.hierarchy_identities(ctx)


def passes_stop_at_the_constant(lib):
    """nns_aggregate stops matching once nagg * bs <= 512 (kNnsCoarseTarget, not PFV_AMG_NNS_COARSE_TARGET): PASSES=6
    leaves the hierarchy of the 300-cell system as it is by default."""
    out = []
    for env in ({}, {"PASSES": 6}):
        A, B, b = NC.user_system(300, 3, 6)
        ctx = _lib.Context(0, lib)
        with environment(env):
            ctx.set_system(A, b)
            ctx.set_near_null_space(B, 3)
            ctx.solve(method="cg", rtol=1e-10, maxit=1, raise_on_fail=False, precond="amg_nns")
            out.append(read_hierarchy(ctx))
    Ha, Hb = out
    assert len(Ha) == len(Hb)
    for a, b in zip(Ha, Hb):
        assert np.array_equal(a["agg"], b["agg"]) and np.array_equal(a["P"], b["P"])
        assert np.array_equal(a["A"].indices, b["A"].indices) and np.array_equal(a["A"].data, b["A"].data)


SHIFT = np.array([1e6, -2e6, 5e5])


def shifted_grid_system(lib, shift):
    """configs[3]-like mechanics (rollers on the low faces, unit traction on top) on the perturbed 5^3 tetrahedral grid,
    its nodes moved by `shift` after the boundary faces were chosen."""
    g = NC.grid_3d(5)
    bf = g.get_all_boundary_faces()
    fc = g.face_centers.copy()
    roll = [bf[fc[axis, bf] < 1e-9] for axis in range(3)]
    top = bf[fc[2, bf] > fc[2].max() - 1e-9]
    if shift is not None:
        g.nodes = g.nodes + np.asarray(shift)[:, None]
        g.compute_geometry()
    bc = pa.BoundaryConditionVectorial(g)
    for axis in range(3):
        bc.is_dir[axis, roll[axis]] = True
        bc.is_neu[axis, roll[axis]] = False
    bv = np.zeros((3, g.num_faces))
    bv[2, top] = -g.face_areas[top]
    return g, NC.mech_data(g, bc=bc, bv=bv.ravel("F"))


def far_from_the_origin(lib):
    """precond="amg_rbm" on the resident system of a grid ~1e6 away from the origin: the device-made modes are
    orthogonalised about the aggregates' centroids, so the identities hold and the solve takes the iterations of the
    grid at the origin (to one)."""
    its = []
    for shift in (None, SHIFT):
        g, data = shifted_grid_system(lib, shift)
        d = pa.Mpsa("mechanics", library=lib)
        d.discretize(g, data)
        with environment({}):
            u, info = d.solve(g, data, rtol=1e-10, precond="amg_rbm")
            assert info["converged"]
            ctx = d._contexts[id(g)][1]
            assert ctx.stats()["amg_nns_modes"] == 6
            nlev = NC.hierarchy_identities(ctx)
            assert nlev >= 2
            if shift is not None:
                assert np.abs(ctx.amg_nns_level(0)["B"][:, 3:]).max() > 1e5  # the rotations the library worked with
        its.append(info["iterations"])
    print("amg_rbm iterations, grid at the origin / moved:", its)
    assert abs(its[0] - its[1]) <= 1, its
    return its


def apply_is_read_only(lib):
    """pfv_amg_nns_apply_device: refused without a hierarchy (the message of pfv_amg_nns_level) and on d_r == d_z; after
    a few applies the solve gives the bits it gave before them, and the read-out is unchanged."""
    A, B, b = NC.user_system(300, 3, 6)
    ctx = _lib.Context(0, lib)
    buf = np.zeros((2, A.shape[0]))
    with environment({}):
        ctx.set_system(A, b)
        ctx.set_near_null_space(B, 3)
        for call in (lambda: ctx.amg_nns_apply_device(buf[0].ctypes.data, buf[1].ctypes.data), lambda: ctx.amg_nns_level(0)):
            try:
                call()
            except _lib.PorefvError as e:
                assert e.status == 4 and "no near-null-space hierarchy" in e.message, (e.status, e.message)
            else:
                raise AssertionError("accepted without a hierarchy")
        x1, i1 = ctx.solve(method="cg", rtol=1e-10, precond="amg_nns")
        assert i1["converged"]
        H1 = read_hierarchy(ctx)
        try:  # (refused before anything is read: host pointers are good enough for the device build too)
            ctx.amg_nns_apply_device(buf[0].ctypes.data, buf[0].ctypes.data)
        except _lib.PorefvError as e:
            assert e.status == 4 and "bad vectors" in e.message, (e.status, e.message)
        else:
            raise AssertionError("d_r == d_z accepted")
        apply_cycle(ctx, lib, vectors(H1)[:4])
        x2, i2 = ctx.solve(method="cg", rtol=1e-10, precond="amg_nns")
        assert i1["iterations"] == i2["iterations"] and np.array_equal(x1, x2)
        for a, c in zip(H1, read_hierarchy(ctx)):
            assert np.array_equal(a["A"].data, c["A"].data) and np.array_equal(a["P"], c["P"])
            assert np.array_equal(a["agg"], c["agg"])
