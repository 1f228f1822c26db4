"""Cases of the Krylov loops past their first iteration (csrc/linalg.inc: krylov_solve with k_cg_tail, k_bicg_tail, k_dot2
and the scalar updates M_CG_BETA / M_RHO_BETA; gmres_solve with gmres_multi_dot, gmres_multi_axpy, the one-thread Givens
and back-substitution kernels; the `M != nullptr` branches of all three around precond_apply), shared by the emulation
suite (test_krylov_emulation.py) and the GPU suite (test_gpu_krylov.py): each takes the library to run on.

Every case runs pfv_solve(method, rtol = 1e-300, maxit = k) -- rtol^2 underflows to zero, so the loop never stops early --
and compares x_k componentwise, relative to ||x_k||_inf, with a numpy.longdouble reference of the same k iterations:

CG, BiCGStab   the loops of krylov_solve restated statement by statement (`cg`, `bicgstab` below), the preconditioner a
               callable: v / diag (what the fused kernels do for M == nullptr) or the block lower-triangular solve.
GMRES          the DEFINING PROPERTY, not the loop: per cycle x += M^-1 V y with y minimising ||r_0 - A M^-1 V y|| over an
               explicitly orthonormalised basis V of the Krylov space of A M^-1 and r_0, the small least-squares problem
               solved by a QR factorisation of A M^-1 V -- no Hessenberg matrix, no rotation (`gmres_property`).  The
               restatement of gmres_solve with its Givens bookkeeping (`gmres_loop`) is only used to measure the noise,
               and in longdouble it has to agree with the property form (test_krylov_emulation.py).

Tolerance, as for the one-iteration cases of tests/_spmv_cases.py: allowed = 8 x noise, noise the largest deviation from
the longdouble reference of the float64 restatement under the summation orders `forward`, `reversed`, `blocks` (GMRES:
also with modified Gram-Schmidt in place of CGS2).  Noise is measured on the references alone, and every case must have
0 < noise <= 1e-13: an input that amplifies rounding beyond that is no pin (it is replaced, the condition stays).

What the call reports: info["rel_residual"] against ||b - A x_ref|| / ||b|| in longdouble, allowed 8 x the deviation of
the figure the float64 restatements report (CG, BiCGStab: the recursive (r, r); GMRES: the true residual that gmres_solve
recomputes on an unconverged return -- the Givens estimate itself never leaves the library on that path).  That noise is
the spread of a single float64 number, so it is taken to be at least u = 2^-53."""
import collections

import numpy as np
import scipy.sparse as sps

from tests._amg_cases import row_of_entries
from tests._spmv_cases import (KRYLOV_FACTOR, KRYLOV_RUNS, LD, UNIT, Handle, _dot, _row_sums, big_spd, environment,
                               krylov_matrix)

HUGE_N = 2048 * 1024 + 2049   # more than kRedBlocks * 256 rows: the grid-stride loops of the tails and k_dot2 run twice
NOISE_MAX = 1e-13
ORDERS = ("forward", "reversed", "blocks")
BLOCK_PTR = (0, 1, 64, 65, 130)  # ... and n: blocks of 1, 63, 1, 65 and n - 130 rows, all below kAmgDenseMax (exact)

Case = collections.namedtuple("Case", "matrix method k restart x0 precond ascending", defaults=(0, False, "jacobi", False))


def label(case):
    out = "%s-%s-k%d" % (case.method, case.matrix.replace(" ", "_"), case.k)
    if case.method == "gmres" and case.restart:
        out += "-m%d" % case.restart
    if case.x0:
        out += "-x0"
    if case.precond != "jacobi":
        out += "-" + case.precond + ("-ascending" if case.ascending else "-shuffled")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# systems

_SYSTEMS = {}


def system(name, ascending=False):
    """(A, b): the matrices of tests/_spmv_cases.py (rows shuffled), `three n<N>` / `huge spd`: the generator of big_spd
    at another size, `diagonal`; ascending: the same matrix with the columns of every row sorted"""
    key = (name, ascending)
    if key not in _SYSTEMS:
        if name == "huge spd" or name.startswith("three n"):
            n = HUGE_N if name == "huge spd" else int(name[7:])
            A = big_spd(n)
            b = np.random.default_rng(900 + n).uniform(-1, 1, n)
        elif name == "diagonal":
            rng = np.random.default_rng(1200)
            A = sps.csr_matrix(sps.diags(rng.choice([-1.0, 1.0], 300) * 10.0 ** rng.uniform(-3, 3, 300)))
            b = rng.uniform(-1, 1, 300)
        else:
            A, b, _ = krylov_matrix(name)
        if ascending:
            A = sps.csr_matrix(A, copy=True)
            A.sort_indices()
        else:
            assert name == "diagonal" or not A.has_sorted_indices, name
        _SYSTEMS[key] = (A, b)
    return _SYSTEMS[key]


def start_vector(n):
    return np.random.default_rng(1100 + n).uniform(-1, 1, n)


# ---------------------------------------------------------------------------------------------------------------------
# the operations of one restatement: a number format and a summation order

_STRUCTURE = {}


def _structure(A):
    """(row of every entry, which entries are diagonal, the common row length when it is at most 8, else 0)"""
    key = id(A)
    if key not in _STRUCTURE:
        row = row_of_entries(A)
        lengths = np.diff(A.indptr)
        width = int(lengths[0]) if lengths[0] <= 8 and np.all(lengths == lengths[0]) else 0
        _STRUCTURE[key] = (A, row, A.indices == row, width)  # (A itself: keeps the id from being reused)
    return _STRUCTURE[key][1:]


class Ops:
    def __init__(self, A, dtype, order):
        self.A = A
        self.n = A.shape[0]
        self.dtype = dtype
        self.order = order
        self.val = A.data.astype(dtype)
        row, on_diag, self.width = _structure(A)
        self.diag = np.zeros(self.n, dtype=dtype)
        self.diag[row[on_diag]] = self.val[on_diag]

    def mv(self, v):
        prod = self.val * v[self.A.indices]
        if self.width:  # rows of one short length: the three orders of _row_sums, column by column
            cols = prod.reshape(self.n, self.width)
            if self.order == "blocks":  # (eight lanes with one product or none each, then the tree over the lanes;
                lanes = [cols[:, j] if j < self.width else None for j in range(8)]  # an empty lane adds an exact zero)
                while len(lanes) > 1:
                    half = len(lanes) // 2
                    lanes = [a if b is None else b if a is None else a + b for a, b in zip(lanes[:half], lanes[half:])]
                return lanes[0]
            if self.order == "reversed":
                cols = cols[:, ::-1]
            s = cols[:, 0].copy()
            for j in range(1, self.width):
                s += cols[:, j]
            return s
        return _row_sums(self.A, prod, self.order)

    def dot(self, a, b):
        return _dot(a, b, self.order)

    def dense_mv(self, M, v):
        if self.order == "reversed":
            return M[:, ::-1] @ v[::-1]
        return M @ v


def jacobi(ops):
    return lambda v: v / ops.diag


def lu_factor(a):
    """Doolittle with partial pivoting, in the number format of `a`"""
    a = a.copy()
    n = a.shape[0]
    piv = np.arange(n)
    for c in range(n):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        if p != c:
            a[[c, p]] = a[[p, c]]
            piv[[c, p]] = piv[[p, c]]
        a[c + 1:, c] /= a[c, c]
        a[c + 1:, c + 1:] -= np.outer(a[c + 1:, c], a[c, c + 1:])
    return a, piv


def lu_solve(lu, piv, rhs):
    y = rhs[piv].copy()
    n = y.size
    for i in range(1, n):
        y[i] -= lu[i, :i] @ y[:i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - lu[i, i + 1:] @ y[i + 1:]) / lu[i, i]
    return y


def block_lower(ops, gauss_seidel):
    """z = M^-1 v, M the block lower-triangular (gauss_seidel) or block diagonal part of A for BLOCK_PTR: forward
    substitution over the blocks, every diagonal block by its LU factors"""
    dense = np.zeros((ops.n, ops.n), dtype=ops.dtype)
    np.add.at(dense, (row_of_entries(ops.A), ops.A.indices), ops.val)
    ptr = list(BLOCK_PTR) + [ops.n]
    blocks = [(p0, p1, lu_factor(dense[p0:p1, p0:p1]), dense[p0:p1, :p0].copy()) for p0, p1 in zip(ptr[:-1], ptr[1:])]

    def apply(v):
        z = np.zeros(ops.n, dtype=ops.dtype)
        for p0, p1, (lu, piv), left in blocks:
            t = v[p0:p1]
            if gauss_seidel and p0:
                t = t - ops.dense_mv(left, z[:p0])
            z[p0:p1] = lu_solve(lu, piv, t)
        return z

    return apply


# ---------------------------------------------------------------------------------------------------------------------
# krylov_solve, statement by statement.  Each returns (x_k, the relative residual the loop reports).

def cg(ops, M, b, x0, k):
    """r = b - A x; z = M^-1 r; p = z; rho = (r, z)                                       [dot2 ... M_START]
       per iteration: v = A p; alpha = rho / (p, v)                                      [spmv_dot, M_CG_ALPHA]
                      x += alpha p; r -= alpha v; z = M^-1 r                             [k_cg_tail]
                      rr = (r, r); beta = (r, z) / rho; rho = (r, z)                     [M_CG_BETA]
                      p = z + beta p"""
    b = b.astype(ops.dtype)
    x = np.zeros_like(b) if x0 is None else x0.astype(ops.dtype)
    r = b if x0 is None else b - ops.mv(x)
    bb = ops.dot(b, b)
    z = M(r)
    p = z
    rho = ops.dot(r, z)
    rr = ops.dot(r, r)
    for _ in range(k):
        v = ops.mv(p)
        alpha = rho / ops.dot(p, v)
        x = x + alpha * p
        r = r - alpha * v
        z = M(r)
        rr = ops.dot(r, r)
        rz = ops.dot(r, z)
        beta = rz / rho
        rho = rz
        p = z + beta * p
    return x, np.sqrt(rr / bb)


def bicgstab(ops, M, b, x0, k):
    """rhat = r = b - A x; p = v = 0; rho = (rhat, r); alpha = omega = 1; beta = 0         [dot2 ... M_START]
       per iteration: p = r + beta (p - omega v); y = M^-1 p
                      v = A y; alpha = rho / (rhat, v)                                   [shard_spmv, M_ALPHA]
                      s = r - alpha v; z = M^-1 s
                      t = A z; omega = (t, s) / (t, t)                                   [spmv_dot, M_OMEGA]
                      x += alpha y + omega z; r = s - omega t                            [k_bicg_tail]
                      rr = (r, r); beta = ((rhat, r) / rho) (alpha / omega); rho = (rhat, r)   [M_RHO_BETA]"""
    b = b.astype(ops.dtype)
    x = np.zeros_like(b) if x0 is None else x0.astype(ops.dtype)
    r = b if x0 is None else b - ops.mv(x)
    bb = ops.dot(b, b)
    rhat = r
    p = np.zeros_like(b)
    v = np.zeros_like(b)
    rr = ops.dot(r, r)
    rho = ops.dot(rhat, r)
    one = ops.dtype(1)
    alpha, omega, beta = one, one, ops.dtype(0)
    for _ in range(k):
        p = r + beta * (p - omega * v)
        y = M(p)
        v = ops.mv(y)
        alpha = rho / ops.dot(rhat, v)
        s = r - alpha * v
        z = M(s)
        t = ops.mv(z)
        omega = ops.dot(t, s) / ops.dot(t, t)
        x = x + (alpha * y + omega * z)
        r = s - omega * t
        rr = ops.dot(r, r)
        rho_new = ops.dot(rhat, r)
        beta = (rho_new / rho) * (alpha / omega)
        rho = rho_new
    return x, np.sqrt(rr / bb)


def cycle_length(restart, maxit):
    """gmres_solve: m = restart > 0 ? min(restart, 200) : 30; m = min(m, max(1, maxit))"""
    m = min(restart, 200) if restart > 0 else 30
    return min(m, max(1, maxit))


def gmres_loop(ops, M, b, x0, k, restart, gram_schmidt="cgs2"):
    """gmres_solve: cycles of m Arnoldi steps (CGS2: two passes of multi-dot and multi-axpy, the coefficients added),
    the Hessenberg column rotated into R and g as it arrives, back-substitution, x += M^-1 V y; the true residual at the
    head of every cycle and on return."""
    dt = ops.dtype
    b = b.astype(dt)
    x = np.zeros_like(b) if x0 is None else x0.astype(dt)
    bb = ops.dot(b, b)
    m = cycle_length(restart, k)
    its = 0
    first = True
    while its < k:
        r = b if (first and x0 is None) else b - ops.mv(x)
        first = False
        beta = np.sqrt(ops.dot(r, r))
        V = [r * (dt(1) / beta)]
        g = np.zeros(m + 2, dtype=dt)
        g[0] = beta
        cs = np.zeros(m, dtype=dt)
        sn = np.zeros(m, dtype=dt)
        R = np.zeros((m + 1, m), dtype=dt)
        j = 0
        while j < m and its < k:
            w = ops.mv(M(V[j]))
            h = np.zeros(j + 2, dtype=dt)
            if gram_schmidt == "cgs2":
                for _ in range(2):
                    c = [ops.dot(V[i], w) for i in range(j + 1)]
                    for i in range(j + 1):
                        w = w - c[i] * V[i]
                        h[i] += c[i]
            else:
                for i in range(j + 1):
                    h[i] = ops.dot(V[i], w)
                    w = w - h[i] * V[i]
            hn = np.sqrt(ops.dot(w, w))
            V.append(w * (dt(1) / hn if hn > 0 else dt(0)))
            for i in range(j):
                a, c = h[i], h[i + 1]
                h[i] = cs[i] * a + sn[i] * c
                h[i + 1] = -sn[i] * a + cs[i] * c
            a = h[j]
            rad = np.sqrt(a * a + hn * hn)
            cs[j], sn[j] = (a / rad, hn / rad) if rad > 0 else (dt(1), dt(0))
            h[j] = rad
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            R[:j + 1, j] = h[:j + 1]
            j += 1
            its += 1
        y = np.zeros(j, dtype=dt)
        for i in range(j - 1, -1, -1):
            t = g[i]
            for q in range(i + 1, j):
                t = t - R[i, q] * y[q]
            y[i] = t / R[i, i] if R[i, i] != 0 else dt(0)
        w = np.zeros_like(b)
        for q in range(j):
            w = w + y[q] * V[q]
        x = x + M(w)
    r = b - ops.mv(x)
    return x, np.sqrt(ops.dot(r, r) / bb)


def _twice_orthogonal(w, Q):
    for _ in range(2):
        for q in Q:
            w = w - np.sum(q * w) * q
    return w


def gmres_property(ops, M, b, x0, k, restart):
    """What GMRES is, cycle by cycle (cycles of m steps, then a partial one): V an orthonormal basis of
    span{r_0, (A M^-1) r_0, ...} (each new direction orthogonalised twice against the earlier ones), W = A M^-1 V,
    W = Q T by Gram-Schmidt (twice), y = T^-1 Q^T r_0, x += M^-1 V y."""
    b = b.astype(ops.dtype)
    x = np.zeros_like(b) if x0 is None else x0.astype(ops.dtype)
    m = cycle_length(restart, k)
    done = 0
    while done < k:
        steps = min(m, k - done)
        r0 = b if (done == 0 and x0 is None) else b - ops.mv(x)
        V, W = [], []
        nxt = r0
        for _ in range(steps):
            nxt = _twice_orthogonal(nxt, V)
            V.append(nxt / np.sqrt(np.sum(nxt * nxt)))
            W.append(ops.mv(M(V[-1])))
            nxt = W[-1]
        Q = []
        T = np.zeros((steps, steps), dtype=ops.dtype)
        for j, w in enumerate(W):
            q = _twice_orthogonal(w, Q)
            q = q / np.sqrt(np.sum(q * q))
            Q.append(q)
            for i in range(j + 1):
                T[i, j] = np.sum(Q[i] * w)
        rhs = np.array([np.sum(q * r0) for q in Q], dtype=ops.dtype)
        y = np.zeros(steps, dtype=ops.dtype)
        for i in range(steps - 1, -1, -1):
            y[i] = (rhs[i] - np.sum(T[i, i + 1:] * y[i + 1:])) / T[i, i]
        upd = np.zeros_like(b)
        for yi, v in zip(y, V):
            upd = upd + yi * v
        x = x + M(upd)
        done += steps
    return x


# ---------------------------------------------------------------------------------------------------------------------
# references

Reference = collections.namedtuple("Reference", "A b x0 x res noise allowed res_noise res_allowed")
_CACHE = {}


def _restate(case, A, b, x0, dtype, order, gram_schmidt="cgs2", loop=True):
    ops = Ops(A, dtype, order)
    M = jacobi(ops) if case.precond == "jacobi" else block_lower(ops, case.precond == "block gs1")
    if case.method == "cg":
        return cg(ops, M, b, x0, case.k)
    if case.method == "bicgstab":
        return bicgstab(ops, M, b, x0, case.k)
    if loop:
        return gmres_loop(ops, M, b, x0, case.k, case.restart, gram_schmidt)
    return gmres_property(ops, M, b, x0, case.k, case.restart), None


def true_residual(A, b, x):
    r = b.astype(LD) - _row_sums(A, A.data.astype(LD) * x.astype(LD)[A.indices], "forward")
    return np.sqrt(np.sum(r * r) / np.sum(b.astype(LD) ** 2))


def reference(case):
    """The longdouble reference of `case`, its noise and the allowances (module docstring)."""
    assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is not wider than float64 on this host"
    if case not in _CACHE:
        A, b = system(case.matrix, case.ascending)
        x0 = start_vector(A.shape[0]) if case.x0 else None
        x, _ = _restate(case, A, b, x0, LD, "forward", loop=False)
        scale = np.abs(x).max()
        res = true_residual(A, b, x)
        runs = [_restate(case, A, b, x0, np.float64, o) for o in ORDERS]
        if case.method == "gmres":
            runs.append(_restate(case, A, b, x0, np.float64, "forward", "mgs"))
        noise = max(float(np.abs(xv.astype(LD) - x).max() / scale) for xv, _ in runs)
        # (one float64 scalar: three or four samples of it can all land on the double next to the longdouble value, as
        # for CG on `spd L16` at k = 2 with 1e-17 -- no float64 figure is owed more than its own rounding, u)
        res_noise = max(UNIT, max(float(abs(LD(rv) - res) / res) for _, rv in runs))
        assert 0 < noise <= NOISE_MAX, (label(case), noise)
        # the reported figure loses digits as the residual falls (its float64 evaluation errs by a few u ||A|| ||x|| /
        # ||b|| absolutely); a case stays a check of it while 8 x noise still resolves five digits
        assert 0 < res_noise <= 1e-6, (label(case), res_noise)
        _CACHE[case] = Reference(A, b, x0, x, res, noise, KRYLOV_FACTOR * noise, res_noise, KRYLOV_FACTOR * res_noise)
    return _CACHE[case]


def loop_gap(case):
    """GMRES: how far the longdouble restatement of gmres_solve is from the property form, relative to ||x_k||_inf"""
    ref = reference(case)
    x = _restate(case, ref.A, ref.b, ref.x0, LD, "forward")[0]
    return float(np.abs(x - ref.x).max() / np.abs(ref.x).max())


# ---------------------------------------------------------------------------------------------------------------------
# the cases

CG_BICGSTAB = [Case(m, method, k) for m, method in KRYLOV_RUNS for k in (2, 3, 6)] + [
    Case("spd L8", "cg", 3, x0=True), Case("ladder L8", "bicgstab", 3, x0=True)]  # r = b - A x0 at the head of the loop
HUGE = [Case("huge spd", "cg", 3), Case("huge spd", "bicgstab", 3)]
HUGE_GMRES = Case("huge spd", "gmres", 3)

GMRES_STEPS = [(1, 0), (2, 0), (8, 0), (9, 0), (17, 0),  # j + 1 = 8 | 9 | 16 | 17: one, two and three passes of kGmresGroup
               (7, 3), (9, 8), (10, 9),                  # full cycles and a partial one
               (4, 50)]                                  # maxit < restart: m = maxit
GMRES = [Case("ladder L8", "gmres", k, m) for k, m in GMRES_STEPS] + [          # n = 200: nb = 1, fewer rows than lanes
    Case("ladder L8", "gmres", 6, 4, x0=True)] + [
    Case(name, "gmres", k, m) for name in ("three n2049", "three n4099")        # nb = 2 and 3, uneven [lo, hi)
    for k, m in ((9, 0), (7, 3))] + [
    Case("big spd", "gmres", 9, 0), Case("big spd", "gmres", 10, 9)]            # nb = 65

BLOCK = [Case(m, method, k, precond="block gs0")
         for m, methods in (("spd L8", ("cg", "bicgstab", "gmres")), ("ladder L8", ("bicgstab", "gmres")))
         for method in methods for k in (1, 2, 5)] + [
    Case(m, method, k, precond="block gs1", ascending=asc)
    for m in ("spd L8", "ladder L8") for method in ("bicgstab", "gmres") for k in (1, 2, 5) for asc in (True, False)]


def check_iterations(lib, case, window="1"):
    """pfv_solve(rtol = 1e-300, maxit = k): k iterations, not converged, x_k and the reported residual within 8 x noise"""
    ref = reference(case)
    n = ref.A.shape[0]
    with environment({"PFV_SPMV_WINDOW": window}):
        with Handle(lib) as h:
            h.set_system(ref.A, ref.b)
            if case.precond != "jacobi":
                h.ctx.set_block_preconditioner(list(BLOCK_PTR) + [n], gauss_seidel=case.precond == "block gs1")
            x, info = h.ctx.solve(method=case.method, rtol=1e-300, maxit=case.k, restart=case.restart, x0=ref.x0,
                                  raise_on_fail=False, precond="jacobi" if case.precond == "jacobi" else "block")
            x = np.array(x, dtype=np.float64)
    scale = float(np.abs(ref.x).max())
    err = np.abs(x.astype(LD) - ref.x) / scale
    worst = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
    dev = float(err[worst])
    res_dev = float(abs(LD(info["rel_residual"]) - ref.res) / ref.res)
    what = "%s (n %d) PFV_SPMV_WINDOW=%s" % (label(case), n, window)
    print("%s: noise %.3e allowed %.3e measured %.3e ratio %.3f | rel_residual %.3e: noise %.3e allowed %.3e measured %.3e"
          % (what, ref.noise, ref.allowed, dev, dev / ref.allowed, float(ref.res), ref.res_noise, ref.res_allowed, res_dev))
    assert info["iterations"] == case.k and not info["converged"], (what, info)
    assert dev <= ref.allowed, "%s: x_k off by %.3e of ||x_k||_inf in row %d: got %r, want %r; allowed %.3e = 8 x noise " \
        "%.3e" % (what, dev, worst, x[worst], float(ref.x[worst]), ref.allowed, ref.noise)
    assert res_dev <= ref.res_allowed, "%s: rel_residual %r, want %r: off by %.3e of it; allowed %.3e = 8 x noise %.3e" % (
        what, info["rel_residual"], float(ref.res), res_dev, ref.res_allowed, ref.res_noise)


# ---------------------------------------------------------------------------------------------------------------------
# edges

def zero_rhs(lib, method):
    """b = 0 with x0 != 0: x = 0 exactly, converged, no iteration"""
    A, _ = system("ladder L8")
    n = A.shape[0]
    with Handle(lib) as h:
        h.set_system(A, np.zeros(n))
        x, info = h.ctx.solve(method=method, rtol=1e-300, maxit=5, x0=start_vector(n), raise_on_fail=False,
                              precond="jacobi")
        x = np.array(x, dtype=np.float64)
    assert info["converged"] and info["iterations"] == 0, (method, info)
    assert not np.any(x), (method, np.flatnonzero(x)[:5])


def diagonal_breakdown(lib, single_entry):
    """GMRES on a diagonal matrix: A M^-1 = I, the Krylov space ends with r_0 (the new direction has norm zero or a few
    roundings, which the `hn > 0 ? 1 / hn : 0` and `d != 0` guards must survive).  x is finite and, every x_i being b_i
    / a_ii up to a few roundings, ||b - A x|| <= 16 u ||b||.  single_entry: b = 4 e_7 -- every product is exact, the
    second direction is exactly zero."""
    A, b = system("diagonal")
    n = A.shape[0]
    if single_entry:
        b = np.zeros(n)
        b[7] = 4.0
    with Handle(lib) as h:
        h.set_system(A, b)
        x, info = h.ctx.solve(method="gmres", rtol=1e-300, maxit=3, raise_on_fail=False, precond="jacobi")
        x = np.array(x, dtype=np.float64)
    assert np.all(np.isfinite(x)), (info, np.flatnonzero(~np.isfinite(x))[:5])
    assert 1 <= info["iterations"] <= 3 and np.isfinite(info["rel_residual"]), info
    r = b.astype(LD) - A.diagonal().astype(LD) * x.astype(LD)
    rel = float(np.sqrt(np.sum(r * r) / np.sum(b.astype(LD) ** 2)))
    print("gmres on a diagonal matrix (%s): %d iterations, ||b - A x|| / ||b|| = %.3e, allowed %.3e"
          % ("b = 4 e_7" if single_entry else "random b", info["iterations"], rel, 16 * UNIT))
    assert rel <= 16 * UNIT, (rel, info)
