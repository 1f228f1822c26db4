"""Cases of the Krylov SpMV family (csrc/spmv_win.inc: k_win_build, k_spmv_win, k_spmv_win_pre; csrc/linalg.inc: k_spmv,
k_spmv_dot), shared by the emulation suite (test_spmv_emulation.py) and the GPU suite (test_gpu_spmv.py): each takes
the library to run on.  The emulation build has no windows: every product there is the sequential row loop of `spmv`.

Every product is judged against two CPU references that know nothing of the library:

exact    matrix values are integers in [-8, 8] without stored zeros, x holds integers in [-16, 16].  Every partial sum
         is an integer far below 2^53, so every summation order, fused or not, gives the same double: the reference is
         an int64 product and y must be equal to it BIT FOR BIT.  A dropped, doubled or misplaced entry in any lane,
         chunk or pass changes an integer.
bounded  values +-10^U(-6, 6) with the signs of the products alternating along a row; the reference is accumulated in
         numpy.longdouble; per row |y_i - yhat_i| <= gamma_{n_i} sum_j |a_ij| |x_j| with gamma_n = n u / (1 - n u),
         u = 2^-53, n_i the row length (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: it holds
         for every order of the n_i products and n_i - 1 additions; an FMA only removes roundings).  No measured
         constant, no margin.

One Krylov iteration (pfv_solve with maxit = 1) is judged against a numpy restatement of the loops of krylov_solve in
longdouble; its tolerance is 8 times the spread of the same restatement in float64 under three summation orders.

A failing check names the matrix, the launch shape (L lanes per row, U chunks in flight, as spmv_win / spmv choose
them), the path, and the first wrong row with its length."""
import ctypes
import math

import numpy as np
import scipy.sparse as sps

import porepy_amd as pa
from porepy_amd import _lib
from tests._amg_cases import environment, row_of_entries, window_columns

LD = np.longdouble
UNIT = 2.0 ** -53          # unit roundoff of float64
MAT = _lib.MAT_USER_SYSTEM
SENTINEL = -7.25
WIN_ROWS = 64              # spmv_win.inc: kWinRows
WIN_MAX = 4096             # spmv_win.inc: kWinMax
RED_BLOCKS = 2048          # linalg.inc: kRedBlocks
KRYLOV_FACTOR = 8.0
U_SWEEP = (0, 1, 2, 3, 4, 5, 6, 7)   # PFV_SPMV_U: 0 = automatic, 7 clamps to 6
U_KERNEL = (2, 3, 4, 5, 6)           # the chunk counts the windowed kernels are instantiated for
LADDER_N = 200


# ---------------------------------------------------------------------------------------------------------------------
# launch shapes as the library chooses them (quoted from spmv_win() and spmv(); only for band checks and messages)

def win_lanes(avg):
    """spmv_win(), f64 values: L = avg <= 20 ? 8 : (avg <= 160 ? 16 : 32)"""
    return 8 if avg <= 20 else (16 if avg <= 160 else 32)


def plain_lanes(avg, env_l=0):
    """spmv(): avg <= 6: 4; <= 20: 8; <= 160: 16; <= 512: 32; else 64 (PFV_SPMV_L overrides)"""
    if env_l:
        return env_l
    return 4 if avg <= 6 else 8 if avg <= 20 else 16 if avg <= 160 else 32 if avg <= 512 else 64


def chunks(avg, lanes, env_u, windowed):
    """U = PFV_SPMV_U or ceil(1.1 avg / L), clamped to 1..6; the windowed launch runs U = 1 with the U = 2 kernel"""
    u = env_u if env_u else int(math.ceil(1.1 * avg / lanes))
    u = max(1, min(6, u))
    return max(u, 2) if windowed else u


# ---------------------------------------------------------------------------------------------------------------------
# patterns

def pattern_from_lengths(lengths, rng, dup_every=0):
    """Square pattern with the given row lengths (capped at n): the diagonal and distinct random columns, shuffled.
    dup_every = k: every k-th row of at least 3 entries stores one of its off-diagonal columns twice."""
    n = len(lengths)
    rows = []
    for i, k in enumerate(lengths):
        k = max(1, min(int(k), n))
        c = rng.choice(n - 1, k - 1, replace=False) if k > 1 else np.zeros(0, dtype=np.int64)
        c = c + (c >= i)
        if dup_every and k >= 3 and i % dup_every == 0:
            c[0] = c[1]
        c = np.concatenate([[i], c])
        rows.append(rng.permutation(c))
    indptr = np.zeros(n + 1, dtype=np.int32)
    indptr[1:] = np.cumsum([r.size for r in rows])
    return indptr, np.concatenate(rows).astype(np.int32)


def ladder_lengths(lanes, n=LADDER_N):
    """1, L-1, L, L+1 and, for every U the kernels are instantiated for, L U - 1, L U, L U + 1, 2 L U + 3 (capped at
    n): the lengths at which a lane gains an entry, a row fills its first U-chunk exactly, and the tail loop of
    k_spmv_win_pre starts / runs a second trip."""
    out = [1, lanes - 1, lanes, lanes + 1]
    for u in U_KERNEL:
        out += [lanes * u - 1, lanes * u, lanes * u + 1, 2 * lanes * u + 3]
    return [min(v, n) for v in out]


LADDER_PAD = {8: 12, 16: 30, 32: 198}  # length of the filling rows: keeps nnz / n in the band of L


def ladder_pattern(lanes, dup=False, n=LADDER_N):
    rng = np.random.default_rng(100 + lanes + (1000 if dup else 0))
    lad = ladder_lengths(lanes, n)
    lengths = lad + lad + [min(n, 6 * lanes + 7)]
    lengths += [LADDER_PAD[lanes]] * (n - len(lengths))
    lengths = list(rng.permutation(lengths))  # (ladder rows in every pass and lane group of a block)
    return pattern_from_lengths(lengths, rng, dup_every=3 if dup else 0)


def tail_pattern(n):
    rng = np.random.default_rng(200 + n)
    return pattern_from_lengths(list(rng.integers(10, 15, n)), rng)


def view_pattern(n=300, per_row=30):
    rng = np.random.default_rng(300)
    return pattern_from_lengths(list(rng.integers(per_row - 3, per_row + 4, n)), rng)


def fixed_pattern(seed, n=300, per_row=25):
    """every row `per_row` entries: two seeds give the same n, indptr and nnz with different columns"""
    rng = np.random.default_rng(seed)
    return pattern_from_lengths([per_row] * n, rng)


BUILDER_N = 262144


def win_hash(col):
    """k_win_build: ((unsigned)col * 2654435761u) >> 19"""
    return ((np.asarray(col, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(19)


def builder_pattern(w, n=BUILDER_N):
    """Every row its diagonal; the 64 rows of block 0 also hold off-diagonal columns so that the block touches exactly
    `w` distinct columns: 0 and n - 1, four runs spaced by 8192 (= the table size of k_win_build) over the whole index
    range, and then the columns whose hash falls into the LAST 200 slots of the table -- 32 candidates per slot, so
    the probe chains are long and run over the end of the table.  Several rows share columns."""
    rng = np.random.default_rng(400 + w)
    assert WIN_ROWS + 1 + 4 * 32 <= w
    chosen = set(range(WIN_ROWS)) | {n - 1}
    runs = [c for off in range(WIN_ROWS, WIN_ROWS + 4) for c in range(off, n, 8192)]
    allc = np.arange(n)
    h = win_hash(allc)
    crowd = allc[h >= 8192 - 200]
    crowd = crowd[np.argsort(h[crowd], kind="stable")]
    for c in runs + list(crowd):
        if len(chosen) >= w:
            break
        chosen.add(int(c))
    assert len(chosen) == w
    off = np.array(sorted(chosen - set(range(WIN_ROWS))), dtype=np.int64)
    off = rng.permutation(off)
    rows = []
    for i in range(WIN_ROWS):
        mine = off[i::WIN_ROWS]
        shared = rng.choice(off, 8, replace=False)  # columns other rows hold too (the table sees them again)
        c = np.unique(np.concatenate([[i], mine, shared]))
        rows.append(rng.permutation(c))
    head = np.concatenate(rows)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:WIN_ROWS + 1] = np.cumsum([r.size for r in rows])
    indptr[WIN_ROWS + 1:] = indptr[WIN_ROWS] + np.arange(1, n - WIN_ROWS + 1)
    indices = np.concatenate([head, np.arange(WIN_ROWS, n)])
    return indptr.astype(np.int32), indices.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# values

def _csr(data, pattern):
    indptr, indices = pattern
    n = indptr.size - 1
    A = sps.csr_matrix((data, indices, indptr), shape=(n, n))  # (no sorting, no merging of repeated columns)
    assert A.nnz == indices.size and np.all(np.diff(indptr) >= 1)
    return A


def _position_in_row(indptr, nnz):
    row = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    return np.arange(nnz) - indptr[:-1].astype(np.int64)[row], row


def exact_values(pattern, seed):
    rng = np.random.default_rng(seed)
    indptr, indices = pattern
    data = rng.integers(1, 9, indices.size) * rng.choice([-1, 1], indices.size)
    pos, row = _position_in_row(indptr, indices.size)
    # a repeated diagonal column may not cancel (pfv_set_system rejects a zero diagonal): diagonals are positive
    data = np.where(indices == row, np.abs(data), data)
    x = rng.integers(-16, 17, indptr.size - 1)
    return _csr(data.astype(np.float64), pattern), x.astype(np.float64)


def bounded_values(pattern, seed):
    rng = np.random.default_rng(seed)
    indptr, indices = pattern
    n = indptr.size - 1
    x = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 6, n)
    pos, _ = _position_in_row(indptr, indices.size)
    sign = np.sign(x[indices]) * np.where(pos % 2 == 0, 1.0, -1.0)  # products alternate in sign: rows cancel
    data = sign * 10.0 ** rng.uniform(-6, 6, indices.size)
    return _csr(data, pattern), x


class Case:
    """one pattern with its exact and its bounded values"""

    def __init__(self, name, pattern, seed=7):
        self.name = name
        self.pattern = pattern
        self.n = pattern[0].size - 1
        self.nnz = pattern[1].size
        self.avg = self.nnz / self.n
        self.exact = exact_values(pattern, seed)
        self.bounded = bounded_values(pattern, seed + 1)

    def row_len(self, r):
        return int(self.pattern[0][r + 1] - self.pattern[0][r])


# ---------------------------------------------------------------------------------------------------------------------
# references

def exact_reference(A, x):
    """int64 product (rows are never empty)"""
    a = A.data.astype(np.int64)
    xi = x.astype(np.int64)
    assert np.array_equal(a, A.data) and np.array_equal(xi, x) and a.size and np.all(a != 0)
    assert np.abs(a).max() <= 8 and np.abs(xi).max() <= 16
    y = np.add.reduceat(a * xi[A.indices], A.indptr[:-1].astype(np.int64))
    assert np.abs(y).max() < 2 ** 53
    return y.astype(np.float64)


def bounded_reference(A, x):
    """(yhat, bound): the rows accumulated in longdouble, and gamma_{n_i} sum_j |a_ij| |x_j|"""
    assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is not wider than float64 on this host"
    prod = A.data.astype(LD) * x.astype(LD)[A.indices]
    ip = A.indptr[:-1].astype(np.int64)
    yhat = np.add.reduceat(prod, ip)
    mag = np.add.reduceat(np.abs(prod), ip)
    nu = np.diff(A.indptr).astype(LD) * LD(UNIT)
    return yhat, nu / (1 - nu) * mag


def first_bad(bad):
    idx = np.flatnonzero(bad)
    return (int(idx[0]), idx.size) if idx.size else (None, 0)


def check_exact(y, A, x, rows, where):
    ref = exact_reference(A, x)[:rows]
    y = np.asarray(y[:rows], dtype=np.float64)
    r, count = first_bad(y.view(np.uint64) != ref.view(np.uint64))
    assert r is None, "%s: exact reference: first wrong row %d (%d entries): got %r, want %r; %d of %d rows wrong" % (
        where, r, A.indptr[r + 1] - A.indptr[r], y[r], ref[r], count, rows)


def check_bounded(y, A, x, rows, where):
    yhat, bound = bounded_reference(A, x)
    err = np.abs(np.asarray(y[:rows], dtype=np.float64).astype(LD) - yhat[:rows])
    r, count = first_bad(~(err <= bound[:rows]))
    assert r is None, "%s: bounded reference: first wrong row %d (%d entries): got %r, want %r, error %.3e > bound " \
        "%.3e; %d of %d rows wrong" % (where, r, A.indptr[r + 1] - A.indptr[r], y[r], float(yhat[r]), float(err[r]),
                                      float(bound[r]), count, rows)


def bound_is_not_vacuous(case):
    """scipy's float64 product and a float64 product with every row summed backwards satisfy the bound, and the bound
    is a rounding-level one: a row that loses its largest product breaks it.  (Entries far below a row's magnitude are
    invisible to this reference by construction; the exact reference is the one that sees every entry.)"""
    A, x = case.bounded
    yhat, bound = bounded_reference(A, x)
    fwd = sps.csr_matrix(A) @ x
    prod = A.data * x[A.indices]
    ip = A.indptr.astype(np.int64)
    row = row_of_entries(A)
    src = ip[row] + ip[row + 1] - 1 - np.arange(A.nnz)
    back = np.array([np.cumsum(prod[src][ip[i]:ip[i + 1]])[-1] for i in range(case.n)])
    for name, y in (("scipy", fwd), ("reversed", back)):
        err = np.abs(y.astype(LD) - yhat)
        assert np.all(err <= bound), (case.name, name, int(np.argmax(err - bound)))
    biggest = np.maximum.reduceat(np.abs(prod), ip[:-1])
    dropped = np.add.reduceat(np.where(np.abs(prod) == biggest[row], 0.0, prod), ip[:-1])
    assert np.all(np.abs(dropped.astype(LD) - yhat) > bound), case.name


def exact_reference_self_check(case):
    """the int64 reference against exact rational arithmetic in Python integers, and against float64 in two orders"""
    A, x = case.exact
    ref = exact_reference(A, x)
    for i in range(case.n):
        s = sum(int(A.data[p]) * int(x[A.indices[p]]) for p in range(A.indptr[i], A.indptr[i + 1]))
        assert float(s) == ref[i], (case.name, i)
    prod = A.data * x[A.indices]
    fwd = np.add.reduceat(prod, A.indptr[:-1].astype(np.int64))
    bwd = np.add.reduceat(prod[::-1], (A.nnz - A.indptr[1:].astype(np.int64))[::-1])[::-1]
    assert fwd.tobytes() == ref.tobytes() and bwd.tobytes() == ref.tobytes(), case.name


# ---------------------------------------------------------------------------------------------------------------------
# running a product

class Handle:
    """One library handle with a user system on it; vectors live where the library expects them (device build: torch
    tensors on the GPU; emulation build: "device" pointers are host pointers)."""

    def __init__(self, lib):
        self.lib = lib
        self.ctx = pa.Context(0, lib)
        self.device = bool(lib.pfv_is_device_build())
        self.n = 0

    def close(self):
        self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_system(self, A, b=None):
        self.n = A.shape[0]
        self.ctx.set_system(A, np.ones(self.n) if b is None else b)

    def product(self, x, nrows=None):
        """nrows = None: pfv_spmv_device (plain kernels); else pfv_spmv_device_rows(nrows) (windowed when a window
        fits) into a y pre-filled with SENTINEL"""
        ctx = self.ctx
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (self.n,)
        if self.device:
            import torch

            xd = torch.from_numpy(x).cuda()
            yd = torch.full((self.n,), SENTINEL, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            xp, yp = xd.data_ptr(), yd.data_ptr()
        else:
            y = np.full(self.n, SENTINEL)
            xp, yp = x.ctypes.data, y.ctypes.data
        if nrows is None:
            ctx._check(self.lib.pfv_spmv_device(ctx._h, MAT, ctypes.c_void_p(xp), ctypes.c_void_p(yp)))
        else:
            ctx.spmv_device_rows(MAT, nrows, xp, yp)
        ctx.sync()
        return yd.cpu().numpy() if self.device else y


def check_sentinel(y, nrows, where):
    tail = y[nrows:]
    r, count = first_bad(tail.view(np.uint64) != np.full(tail.size, SENTINEL).view(np.uint64))
    assert r is None, "%s: row %d beyond nrows = %d was written (%r); %d such rows" % (
        where, nrows + (r or 0), nrows, tail[r or 0], count)


def where_of(case, windowed, env_u=0, env_l=0, extra=""):
    lanes = win_lanes(case.avg) if windowed else plain_lanes(case.avg, env_l)
    return "%s (n %d, nnz/n %.1f): %s L=%d U=%d%s" % (
        case.name, case.n, case.avg, "windowed" if windowed else "plain", lanes,
        chunks(case.avg, lanes, env_u, windowed), extra)


def both_paths(h, case, kind, env_u=0, env_l=0, paths=(True, False), extra=""):
    """the product of the system on `h` through pfv_spmv_device_rows(n) and pfv_spmv_device, against reference `kind`"""
    A, x = getattr(case, kind)
    check = check_exact if kind == "exact" else check_bounded
    for windowed in paths:
        y = h.product(x, case.n if windowed else None)
        check(y, A, x, case.n, where_of(case, windowed, env_u, env_l, extra))


# ---------------------------------------------------------------------------------------------------------------------
# product cases

def ladder_case(lanes, dup=False):
    case = Case("ladder L%d%s" % (lanes, " with a repeated column per row" if dup else ""), ladder_pattern(lanes, dup))
    # the band of L, from spmv_win (avg <= 20: 8, <= 160: 16, else 32) and spmv (the same above avg = 6)
    lo, hi = {8: (6, 20), 16: (20, 160), 32: (160, 512)}[lanes]
    assert lo < case.avg <= hi, (lanes, case.avg)
    assert win_lanes(case.avg) == lanes and plain_lanes(case.avg) == lanes
    present = set(np.diff(case.pattern[0]).tolist())
    assert set(ladder_lengths(lanes)) | {min(LADDER_N, 6 * lanes + 7)} <= present
    if dup:
        A = case.exact[0]
        assert any(np.unique(A.indices[A.indptr[i]:A.indptr[i + 1]]).size < A.indptr[i + 1] - A.indptr[i]
                   for i in range(case.n))
    return case


def ladder_products(lib, lanes):
    """Row lengths around every chunk boundary of every instantiated (L, U), both references, PFV_SPMV_U swept, through
    the windowed and the plain entry point; the short-row matrix also through the plain kernel with 4 and 64 lanes.
    The variant with a column stored twice in a row: pfv_set_system accepts it (it sums the diagonal's copies), the
    window holds the column once and both entries point at it."""
    for dup in (False, True):
        case = ladder_case(lanes, dup)
        for kind in (("exact",) if dup else ("exact", "bounded")):
            with Handle(lib) as h:
                h.set_system(getattr(case, kind)[0])
                for u in U_SWEEP:
                    with environment({"PFV_SPMV_U": u}):
                        both_paths(h, case, kind, env_u=u)
                if lanes == 8 and not dup:
                    for env_l in (4, 64):
                        for u in (0, 3):
                            with environment({"PFV_SPMV_L": env_l, "PFV_SPMV_U": u}):
                                both_paths(h, case, kind, env_u=u, env_l=env_l, paths=(False,))


TAIL_SIZES = (1, 7, 8, 9, 63, 64, 65, 127, 129)


def tail_products(lib, n):
    """About 12 entries per row (capped at n): a partial last block of 64 rows and partial passes of 256 / L rows --
    L = 8 as both entry points choose it, and the plain kernel with PFV_SPMV_L = 32 and PFV_SPMV_U = 2 (the windowed
    launch has no switch for L: it follows nnz / n alone)."""
    case = Case("tails n%d" % n, tail_pattern(n))
    assert case.avg <= 20
    for kind in ("exact", "bounded"):
        with Handle(lib) as h:
            h.set_system(getattr(case, kind)[0])
            both_paths(h, case, kind)
            with environment({"PFV_SPMV_L": 32, "PFV_SPMV_U": 2}):
                both_paths(h, case, kind, env_u=2, env_l=32, paths=(False,))


VIEW_ROWS = (1, 63, 64, 65, 299, 300)


def row_view(lib):
    """pfv_spmv_device_rows with nrows < n on one handle, ascending then descending (every change of nrows rebuilds the
    window; the second call with the same nrows takes the kept one): rows [0, nrows) match the reference, rows
    [nrows, n) keep the sentinel bit for bit."""
    case = Case("row view", view_pattern())
    assert int(case.pattern[1][: case.pattern[0][1]].max()) > 1  # (columns reach beyond the view)
    for kind in ("exact", "bounded"):
        A, x = getattr(case, kind)
        check = check_exact if kind == "exact" else check_bounded
        with Handle(lib) as h:
            h.set_system(A)
            for nrows in VIEW_ROWS + VIEW_ROWS[::-1]:
                for call in (1, 2):
                    y = h.product(x, nrows)
                    where = "%s: nrows = %d (call %d)" % (where_of(case, True), nrows, call)
                    check(y, A, x, nrows, where)
                    check_sentinel(y, nrows, where)


BUILDER_W = (1000, 1024, 1025, 3000, 4096, 4097)


def builder_case(w):
    case = Case("window builder W%d" % w, builder_pattern(w))
    A = case.exact[0]
    assert window_columns(A) == w
    assert np.unique(A.indices[: A.indptr[WIN_ROWS]]).size == w
    return case


def builder_expectation(w, env):
    """the line win_build reports under PFV_DEBUG_WIN=1 (None: no window is attempted)"""
    if str(env.get("PFV_SPMV_WINDOW", "1")) == "0":
        return None
    stride = int(env.get("PFV_WIN_STRIDE", 1024))
    if str(env.get("PFV_WIN_ONEPASS", "1")) != "0" and w <= stride:
        return "win_build (one pass, stride %d): rows %d" % (stride, BUILDER_N), "wmax %d" % w
    if w <= WIN_MAX:
        return "win_build: rows %d" % BUILDER_N, "wmax %d overflow 0" % w
    return "win_build: rows %d" % BUILDER_N, "overflow 1"


def builder_products(lib, w, env, read_stderr=None):
    """Block 0 touches exactly W distinct columns; the builder must take the layout `builder_expectation` names (read
    from its PFV_DEBUG_WIN line when `read_stderr` is given: the device build) and the product must match both
    references on either entry point."""
    case = builder_case(w)
    env = dict(env)
    env["PFV_DEBUG_WIN"] = 1
    extra = " W=%d %s" % (w, " ".join("%s=%s" % kv for kv in sorted(env.items())))
    with environment(env):
        for kind in ("exact", "bounded"):
            with Handle(lib) as h:
                h.set_system(getattr(case, kind)[0])
                if read_stderr:
                    read_stderr()
                both_paths(h, case, kind, paths=(True,), extra=extra)
                if read_stderr:
                    err = read_stderr()
                    lines = [l for l in err.splitlines() if l.startswith("win_build")]
                    want = builder_expectation(w, env)
                    if want is None:
                        assert not lines, (extra, lines)
                    else:
                        assert len(lines) == 1 and lines[0].startswith(want[0]) and want[1] in lines[0], (extra, want, lines)
                both_paths(h, case, kind, paths=(True, False), extra=extra + " (window kept)")


def cache_invalidation(lib):
    """Two systems with the same n, indptr and nnz and different columns on one handle, then PFV_SPMV_WINDOW off and on
    again with a fresh set_system each time: every product belongs to the matrix set last."""
    c1 = Case("fixed rows, pattern 1", fixed_pattern(501), seed=11)
    c2 = Case("fixed rows, pattern 2", fixed_pattern(502), seed=13)
    assert np.array_equal(c1.pattern[0], c2.pattern[0]) and not np.array_equal(c1.pattern[1], c2.pattern[1])
    with Handle(lib) as h:
        step = 0
        for flag, case in (("1", c1), ("1", c2), ("0", c1), ("1", c2), ("0", c2), ("1", c1)):
            for kind in ("exact", "bounded"):
                step += 1
                with environment({"PFV_SPMV_WINDOW": flag}):
                    h.set_system(getattr(case, kind)[0])
                    both_paths(h, case, kind, extra=" step %d PFV_SPMV_WINDOW=%s" % (step, flag))


def non_finite(lib):
    """+Inf in one x[j]: the rows without an entry in column j are bit-identical to the finite run (the masked lanes
    multiply 0.0 by x[first column of their own row], never by a column the row does not hold); the rows with one are
    Inf or NaN.  Nothing more is asserted."""
    case = Case("row view", view_pattern())
    A, x = case.exact
    j = int(A.indices[A.indptr[5]])  # the FIRST stored column of row 5: what that row's masked lanes read
    xi = x.copy()
    xi[j] = np.inf
    holds = np.zeros(case.n, dtype=bool)
    holds[row_of_entries(A)[A.indices == j]] = True
    assert 1 <= holds.sum() < case.n
    with Handle(lib) as h:
        h.set_system(A)
        for u in (0, 6):
            with environment({"PFV_SPMV_U": u}):
                for windowed in (True, False):
                    where = where_of(case, windowed, u) + " x[%d] = Inf" % j
                    fin = h.product(x, case.n if windowed else None)
                    inf = h.product(xi, case.n if windowed else None)
                    check_exact(fin, A, x, case.n, where)
                    r, count = first_bad((fin.view(np.uint64) != inf.view(np.uint64)) & ~holds)
                    assert r is None, "%s: row %d (%d entries) holds no entry in column %d and moved: %r -> %r; %d " \
                        "such rows" % (where, r, case.row_len(r), j, fin[r], inf[r], count)
                    r, count = first_bad(np.isfinite(inf) & holds)
                    assert r is None, "%s: row %d holds column %d and stayed finite: %r; %d such rows" % (
                        where, r, j, inf[r], count)


# ---------------------------------------------------------------------------------------------------------------------
# one Krylov iteration

def shuffle_rows(A, rng):
    A = sps.csr_matrix(A)
    order = np.argsort(row_of_entries(A) + rng.random(A.nnz))
    return sps.csr_matrix((A.data[order], A.indices[order], A.indptr), shape=A.shape)


def dominant(pattern, seed):
    """the pattern with values in (-1, 1) and the diagonal 1 + the row's absolute off-diagonal sum"""
    rng = np.random.default_rng(seed)
    indptr, indices = pattern
    data = rng.uniform(-1, 1, indices.size)
    _, row = _position_in_row(indptr, indices.size)
    diag = indices == row
    off = np.bincount(row[~diag], weights=np.abs(data[~diag]), minlength=indptr.size - 1)
    data[diag] = 1.0 + off[row[diag]]
    return _csr(data, pattern)


def spd_from(pattern, seed):
    """symmetric, strictly diagonally dominant with a positive diagonal (so SPD) on the symmetrised off-diagonal pattern,
    columns shuffled inside the rows"""
    rng = np.random.default_rng(seed)
    A = _csr(np.ones(pattern[1].size), pattern)
    off = sps.triu(A + A.T, 1).tocsr()
    off.data = -rng.uniform(0.1, 1.0, off.nnz)
    S = off + off.T
    S = sps.csr_matrix(S + sps.diags(1.0 + np.asarray(abs(S).sum(axis=1)).ravel()))
    return shuffle_rows(S, rng)


def big_spd(n=None):
    """n = 64 * 2049 + 5 rows of 3 entries (periodic second difference plus a random positive shift): 2050 row blocks
    for the windowed product and 4099 row groups for k_spmv_dot, more than kRedBlocks partial sums either way.  (Another
    `n`: the same generator at that size, for tests/_krylov_cases.py.)"""
    n = WIN_ROWS * (RED_BLOCKS + 1) + 5 if n is None else n
    rng = np.random.default_rng(600)
    w = rng.uniform(0.5, 1.5, n)  # coupling of i and i + 1 (mod n)
    i = np.arange(n)
    S = sps.coo_matrix((np.concatenate([-w, -w]), (np.concatenate([i, (i + 1) % n]), np.concatenate([(i + 1) % n, i]))),
                       shape=(n, n)).tocsr()
    S = sps.csr_matrix(S + sps.diags(w + np.roll(w, 1) + rng.uniform(0.1, 1.0, n)))
    assert np.all(np.diff(S.indptr) == 3)
    return shuffle_rows(S, rng)


KRYLOV_MATRICES = ("ladder L8", "ladder L16", "ladder L32", "spd L8", "spd L16", "big spd")
KRYLOV_RUNS = [(m, "bicgstab") for m in ("ladder L8", "ladder L16", "ladder L32", "big spd")] + \
              [(m, "cg") for m in ("spd L8", "spd L16", "big spd")]
_SPD_PAD = {8: 3, 16: 10}  # filling rows of the SPD variants: the symmetrised pattern stays in the band of L


def krylov_matrix(name):
    if name.startswith("ladder L"):
        lanes = int(name[8:])
        A = dominant(ladder_pattern(lanes), 700 + lanes)
    elif name.startswith("spd L"):
        lanes = int(name[5:])
        rng = np.random.default_rng(800 + lanes)
        lad = ladder_lengths(lanes)
        lengths = lad + [min(LADDER_N, 6 * lanes + 7)]
        lengths += [_SPD_PAD[lanes]] * (LADDER_N - len(lengths))
        A = spd_from(pattern_from_lengths(list(rng.permutation(lengths)), rng), 810 + lanes)
        assert abs(A - A.T).max() == 0
    else:
        lanes = 8
        A = big_spd()
    n = A.shape[0]
    assert win_lanes(A.nnz / n) == lanes, (name, A.nnz / n)
    b = np.random.default_rng(900 + n).uniform(-1, 1, n)
    return A, b, lanes


def _row_sums(A, prod, order):
    ip = A.indptr.astype(np.int64)
    if order == "reversed":
        row = row_of_entries(A)
        prod = prod[ip[row] + ip[row + 1] - 1 - np.arange(A.nnz)]
    if order == "blocks":  # eight lanes stride through the row, then a tree over the lanes
        pos, row = _position_in_row(A.indptr, A.nnz)
        lanes = np.zeros((A.shape[0], 8), dtype=prod.dtype)
        np.add.at(lanes, (row, pos % 8), prod)
        s = lanes[:, :4] + lanes[:, 4:]
        s = s[:, :2] + s[:, 2:]
        return s[:, 0] + s[:, 1]
    return np.add.reduceat(prod, ip[:-1])


def _dot(a, b, order):
    p = a * b
    if order == "forward":
        return np.cumsum(p)[-1]
    if order == "reversed":
        return np.cumsum(p[::-1])[-1]
    part = np.add.reduceat(p, np.arange(0, p.size, WIN_ROWS))  # one partial per block of 64 rows, then pairwise
    while part.size > 1:
        if part.size % 2:
            part = np.concatenate([part, np.zeros(1, dtype=part.dtype)])
        part = part[0::2] + part[1::2]
    return part[0]


def one_iteration(A, b, method, dtype, order="forward"):
    """x after ONE iteration of krylov_solve (linalg.inc) from x = 0 with the Jacobi preconditioner fused into the
    vector kernels (M == nullptr), statement by statement:

    CG        r = b; z = r / diag; p = z; rho = (r, z)                              [dot2 ... M_START]
              v = A p; alpha = rho / (p, v)                                         [spmv_dot(p, v, w = p, 1, M_CG_ALPHA)]
              x = alpha p                                                           [k_cg_tail]
    BiCGStab  rhat = r = b; p = v = 0; rho = (rhat, r); alpha = omega = 1, beta = 0 [dot2 ... M_START]
              p = r + beta (p - omega v) = r; y = p / diag                          (right preconditioning)
              v = A y; alpha = rho / (rhat, v)                                      [shard_spmv(y, v, w = rhat, 1, M_ALPHA)]
              s = r - alpha v; z = s / diag
              t = A z; omega = (t, s) / (t, t)                                      [spmv_dot(z, t, w = s, 2, M_OMEGA)]
              x = alpha y + omega z                                                 [k_bicg_tail]"""
    A = sps.csr_matrix(A)
    val = A.data.astype(dtype)
    b = b.astype(dtype)
    diag = np.zeros(A.shape[0], dtype=dtype)
    on_diag = A.indices == row_of_entries(A)
    diag[A.indices[on_diag]] = val[on_diag]

    def mv(v):
        return _row_sums(A, val * v[A.indices], order)

    r = b
    if method == "cg":
        z = r / diag
        p = z
        rho = _dot(r, z, order)
        v = mv(p)
        alpha = rho / _dot(p, v, order)
        return alpha * p
    rhat = r
    rho = _dot(rhat, r, order)
    y = r / diag
    v = mv(y)
    alpha = rho / _dot(rhat, v, order)
    s = r - alpha * v
    z = s / diag
    t = mv(z)
    omega = _dot(t, s, order) / _dot(t, t, order)
    return alpha * y + omega * z


_KRYLOV_CACHE = {}


def krylov_reference(name, method):
    """(A, b, lanes, x1 in longdouble, noise, allowed): noise is the largest componentwise deviation of the float64
    restatement under three summation orders from the longdouble one, relative to ||x1||_inf; allowed = 8 noise (the
    device sums in yet another order -- per-block partials -- and contracts to FMA)."""
    key = (name, method)
    if key not in _KRYLOV_CACHE:
        A, b, lanes = krylov_matrix(name)
        ref = one_iteration(A, b, method, LD)
        scale = float(np.abs(ref).max())
        noise = max(float(np.abs(one_iteration(A, b, method, np.float64, o).astype(LD) - ref).max()) / scale
                    for o in ("forward", "reversed", "blocks"))
        assert 0 < noise <= 16 * A.shape[0] * UNIT, (name, method, noise)  # (a-priori: a handful of dots of length n)
        _KRYLOV_CACHE[key] = (A, b, lanes, ref, noise, KRYLOV_FACTOR * noise)
    return _KRYLOV_CACHE[key]


def krylov_iteration(lib, name, method, window):
    """pfv_solve(method, rtol = 1e-300, maxit = 1) from zero with Jacobi: x1 against the longdouble restatement.  A wrong
    (t, t), (t, s), (rhat, v) or (p, A p) moves x1 at relative order one."""
    A, b, lanes, ref, noise, allowed = krylov_reference(name, method)
    n = A.shape[0]
    with environment({"PFV_SPMV_WINDOW": window}):
        with Handle(lib) as h:
            h.set_system(A, b)
            x, info = h.ctx.solve(method=method, rtol=1e-300, maxit=1, raise_on_fail=False, precond="jacobi")
            x = np.array(x, dtype=np.float64)
    assert info["iterations"] == 1 and not info["converged"], info
    scale = float(np.abs(ref).max())
    err = np.abs(x.astype(LD) - ref) / scale
    worst = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
    dev = float(err[worst])
    avg = A.nnz / n
    print("one %s iteration, %s (n %d, nnz/n %.1f, L=%d U=%d), PFV_SPMV_WINDOW=%s: noise %.3e allowed %.3e measured %.3e"
          % (method, name, n, avg, lanes, chunks(avg, lanes, 0, str(window) == "1"), window, noise, allowed, dev))
    assert dev <= allowed, "one %s iteration, %s (n %d, L=%d U=%d) PFV_SPMV_WINDOW=%s: x1 off by %.3e of ||x1||_inf " \
        "in row %d (%d entries): got %r, want %r; allowed %.3e = 8 x noise %.3e" % (
            method, name, n, lanes, chunks(avg, lanes, 0, str(window) == "1"), window, dev, worst,
            A.indptr[worst + 1] - A.indptr[worst], x[worst], float(ref[worst]), allowed, noise)


# ---------------------------------------------------------------------------------------------------------------------
# the windowed f64 kernels without the preloading twin (PFV_SPMV_PRELOAD is read once per process: a child runs these)

PRELOAD_OFF_U = (2, 5)


def preload_off_report(lib):
    """the ladder matrices through pfv_spmv_device_rows(n), exact reference only: one record per (L, U)"""
    out = []
    for lanes in (8, 16, 32):
        case = ladder_case(lanes)
        A, x = case.exact
        ref = exact_reference(A, x)
        with Handle(lib) as h:
            h.set_system(A)
            for u in PRELOAD_OFF_U:
                with environment({"PFV_SPMV_U": u}):
                    y = h.product(x, case.n)
                r, count = first_bad(y.view(np.uint64) != ref.view(np.uint64))
                out.append({"matrix": case.name, "L": lanes, "U": u, "wrong_rows": count, "first_wrong_row": r,
                            "row_entries": None if r is None else case.row_len(r),
                            "got": None if r is None else repr(float(y[r])),
                            "want": None if r is None else repr(float(ref[r]))})
    return out
