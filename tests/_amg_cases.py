"""Cases of the plain aggregation AMG (PFV_PRECOND_AMG; csrc/amg.inc), shared by the emulation suite
(test_amg_emulation.py) and the GPU suite (test_gpu_amg.py): each takes the library to run on.

Everything is judged from the read-out of the hierarchy (Context.amg_level): the setup identities are recomputed on the
host in numpy.longdouble, and the cycle is evaluated by a plain reference written from the header comment of amg.inc.

Tolerances (none comes from the library's output): every quantity is evaluated twice on the host, in longdouble and in
float64 with the columns of every row reversed (another summation order).  The library sums a row in a lane tree in
float64 (FP32 -> FP64 conversion is exact), so its error is of the class of the reordered float64 evaluation: it gets
FACTOR = 16 times the largest float64-vs-longdouble difference of the case, and no bound may exceed HARD = 1e-10."""
import contextlib
import os

import numpy as np
import scipy.sparse as sps

import porepy_amd as pa
from porepy_amd import _lib

LD = np.longdouble
EPS = np.finfo(np.float64).eps
FACTOR = 16.0
HARD = 1e-10


@contextlib.contextmanager
def environment(env):
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------------------------------------------------------------
# systems

def tet_grid(n, perturb=None):
    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    return pa.perturb_interior_nodes(g, (0.25 / n) if perturb is None else perturb)


def cart_grid(dims):
    g = pa.CartGrid(list(dims), [1.0] * len(dims))
    g.compute_geometry()
    return g


class FlowSystem:
    """MPFA system of a grid, resident on its handle; ``set_values`` re-discretizes with other permeabilities."""

    def __init__(self, lib, g, seed=2, sigma=0.5):
        self.lib, self.g = lib, g
        self.rng = np.random.default_rng(seed)
        self.sc = np.exp(sigma * self.rng.standard_normal(g.num_cells))
        bf = g.get_all_boundary_faces()
        xf = g.face_centers[0, bf]
        dirf = bf[(xf < 1e-9) | (xf > g.nodes[0].max() - 1e-9)]
        bv = np.zeros(g.num_faces)
        bv[dirf] = g.face_centers[0, dirf]
        self.data = pa.initialize_data({}, "flow", {"second_order_tensor": self._tensor(self.sc),
                                                    "bc": pa.BoundaryCondition(g, dirf, ["dir"] * dirf.size),
                                                    "bc_values": bv})
        self.d = pa.Mpfa("flow", library=lib)
        self.assemble()

    def _tensor(self, sc):
        kw = dict(kxx=sc, kyy=5 * sc, kxy=0.4 * sc)
        if self.g.dim == 3:
            kw.update(kzz=0.2 * sc, kyz=0.1 * sc)
        return pa.SecondOrderTensor(**kw)

    def assemble(self, rebuild=False):
        par = self.data[pa.PARAMETERS]["flow"]
        par.pop("hip_rebuild_topology", None)
        if rebuild:
            par["hip_rebuild_topology"] = True
        self.d.discretize(self.g, self.data)
        self.A, self.b = self.d.assemble_matrix_rhs(self.g, self.data)
        self.A = sps.csr_matrix(self.A)
        self.ctx = self.d.context(self.g)
        self.n = self.A.shape[0]

    def set_values(self, sc, rebuild=False):
        self.sc = sc
        self.data[pa.PARAMETERS]["flow"]["second_order_tensor"] = self._tensor(sc)
        self.assemble(rebuild)


class MechSystem:
    """MPSA system (bs = nd unknowns per cell): bottom clamped, Lame parameters with a mild contrast."""

    def __init__(self, lib, g, seed=1):
        rng = np.random.default_rng(seed)
        nc, nd = g.num_cells, g.dim
        het = np.where(g.cell_centers[0] > 0.5, 20.0, 1.0)
        C = pa.FourthOrderTensor(het * (1 + rng.random(nc)), het * (1 + rng.random(nc)))
        bc = pa.BoundaryConditionVectorial(g)
        bf = g.get_all_boundary_faces()
        bot = bf[g.face_centers[nd - 1, bf] < 1e-9]
        bc.is_dir[:, bot] = True
        bc.is_neu[:, bot] = False
        self.data = pa.initialize_data({}, "mechanics", {"fourth_order_tensor": C, "bc": bc,
                                                         "bc_values": np.zeros(nd * g.num_faces)})
        self.d = pa.Mpsa("mechanics", library=lib)
        self.d.discretize(g, self.data)
        A, self.b = self.d.assemble_matrix_rhs(g, self.data)
        self.A = sps.csr_matrix(A)
        self.ctx = self.d.context(g)
        self.n = self.A.shape[0]


class UserSystem:
    def __init__(self, lib, A, seed=0):
        self.A = A
        self.n = A.shape[0]
        self.b = np.random.default_rng(seed).standard_normal(self.n)
        self.ctx = _lib.Context(0, lib)
        self.ctx.set_system(A, self.b)


def shuffled_columns(A, rng):
    A = sps.csr_matrix(A)
    A.sort_indices()
    perm = np.concatenate([rng.permutation(np.arange(A.indptr[i], A.indptr[i + 1])) for i in range(A.shape[0])])
    return sps.csr_matrix((A.data[perm], A.indices[perm], A.indptr), shape=A.shape)


def graph_matrix(n, rng, k=5, shift=0.05):
    """Diagonally dominant M-matrix-like system on the k-nearest-neighbour graph of random points in the plane, numbered
    along x (local), with random weights over two decades."""
    pts = rng.random((n, 2))
    pts = pts[np.argsort(pts[:, 0])]
    rows, cols = [], []
    cell = max(1, int(np.sqrt(n / 12.0)))
    key = (np.floor(pts[:, 0] * cell) * cell + np.floor(pts[:, 1] * cell)).astype(int)
    for c in np.unique(key):
        near = np.flatnonzero(np.abs(pts[:, 0] - (c // cell + 0.5) / cell) <= 1.5 / cell)
        mine = np.flatnonzero(key == c)
        d = np.linalg.norm(pts[mine][:, None, :] - pts[near][None, :, :], axis=2)
        nb = near[np.argsort(d, axis=1)[:, 1:k + 1]]
        rows.append(np.repeat(mine, nb.shape[1]))
        cols.append(nb.ravel())
    r, c = np.concatenate(rows), np.concatenate(cols)
    G = sps.coo_matrix((np.ones(r.size), (r, c)), shape=(n, n)).tocsr()
    G = ((G + G.T) > 0).astype(float).tocoo()
    w = np.exp(2.3 * rng.random(G.nnz))
    W = sps.coo_matrix((w, (G.row, G.col)), shape=(n, n)).tocsr()
    W = 0.5 * (W + W.T)
    return sps.csr_matrix(sps.diags(np.asarray(W.sum(axis=1)).ravel() * (1 + shift)) - W)


def edge_case_matrix(n=1500, hub_degree=700, seed=7):
    """User CSR system with unsorted columns, one row that holds only its diagonal (a singleton aggregate: the last
    row, which also puts it on the tail row block) and a hub row with several hundred entries."""
    rng = np.random.default_rng(seed)
    A = graph_matrix(n - 1, rng).tolil()
    hub = 17
    others = rng.choice(np.setdiff1d(np.arange(n - 1), [hub]), hub_degree, replace=False)
    for j in others:
        w = 0.5 * (1 + rng.random())  # (strong enough to survive the strength filter)
        A[hub, j] -= w
        A[j, hub] -= w
        A[hub, hub] += 1.05 * w
        A[j, j] += 1.05 * w
    A = sps.bmat([[A.tocsr(), None], [None, sps.csr_matrix(np.array([[3.0]]))]], format="csr")
    return shuffled_columns(A, rng), hub


def no_locality_matrix(clusters=900, per_row=60, seed=3):
    """A block of 64 rows touches more than 4096 distinct columns (about 120 random ones per row): no SpMV window fits.
    Rows come in randomly numbered clusters of 8 with strong couplings inside (the three pairwise passes find them: one
    coarsening to about `clusters` rows) and random couplings, a tenth as strong, to everything else -- above the
    strength filter, so the operator of level 0 stays above the size from which its window is tried."""
    rng = np.random.default_rng(seed)
    n = 8 * clusters
    R = sps.random(n, n, density=per_row / n, random_state=seed, format="csr")
    R.data = 0.5 + 0.5 * R.data
    R.setdiag(0.0)
    R.eliminate_zeros()
    perm = rng.permutation(n)
    Pm = sps.csr_matrix((np.ones(n), (perm, np.arange(n))), shape=(n, n))
    K = sps.kron(sps.eye(clusters), 8.0 * (np.ones((8, 8)) - np.eye(8)))
    R = sps.csr_matrix(0.5 * (R + R.T) + Pm @ K @ Pm.T)
    return sps.csr_matrix(sps.diags(np.asarray(R.sum(axis=1)).ravel() * 1.1 + rng.random(n)) - R)


def window_columns(M, rows=64):
    """largest number of distinct columns a block of `rows` rows touches (what the SpMV windows hold at most 4096 of)"""
    return max(np.unique(M.indices[M.indptr[r]:M.indptr[min(r + rows, M.shape[0])]]).size
               for r in range(0, M.shape[0], rows))


def stalled_matrix(clusters=1200, seed=5):
    """Disjoint triangles with couplings between them far below the strength filter: one level of coarsening (every
    triangle an aggregate), then nothing left to match on `clusters` > kAmgDenseMax rows -- the coarsest level is
    smoothed (Jacobi fallback) instead of inverted."""
    rng = np.random.default_rng(seed)
    n = 3 * clusters
    r, c, v = [], [], []
    for a, b in ((0, 1), (1, 2), (0, 2)):
        i = 3 * np.arange(clusters) + a
        j = 3 * np.arange(clusters) + b
        w = 1 + rng.random(clusters)
        r += [i, j]
        c += [j, i]
        v += [-w, -w]
    i = 3 * np.arange(clusters - 1)  # weak chain between neighbouring triangles
    w = 1e-3 * (1 + rng.random(clusters - 1))
    r += [i, i + 3]
    c += [i + 3, i]
    v += [-w, -w]
    W = sps.coo_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(n, n)).tocsr()
    return sps.csr_matrix(W + sps.diags(-np.asarray(W.sum(axis=1)).ravel() * 1.2))


# ---------------------------------------------------------------------------------------------------------------------
# read-out and application

def read_hierarchy(ctx):
    lev0 = ctx.amg_level(0)
    return [lev0] + [ctx.amg_level(l) for l in range(1, lev0["levels"])]


def apply_cycle(ctx, lib, R):
    """pfv_amg_apply_device on the rows of R.  Emulation build: "device" pointers are host pointers."""
    R = np.ascontiguousarray(np.atleast_2d(R), dtype=np.float64)
    if lib.pfv_is_device_build():
        import torch

        r = torch.from_numpy(R).cuda()
        z = torch.zeros_like(r)
        torch.cuda.synchronize()
        for i in range(R.shape[0]):
            ctx.amg_apply_device(r[i].data_ptr(), z[i].data_ptr())
        ctx.sync()
        return z.cpu().numpy()
    Z = np.zeros_like(R)
    for i in range(R.shape[0]):
        ctx.amg_apply_device(R[i].ctypes.data, Z[i].ctypes.data)
    ctx.sync()
    return Z


def row_of_entries(M):
    return np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))


def reversed_rows(M):
    """The same matrix with the entries of every row stored in the opposite order."""
    ip = M.indptr.astype(np.int64)
    row = row_of_entries(M)
    src = ip[row] + ip[row + 1] - 1 - np.arange(M.nnz)
    return sps.csr_matrix((M.data[src], M.indices[src], M.indptr), shape=M.shape)


def unknown_map(agg, bs):
    """fine unknown -> coarse unknown of P = P_cell (x) I_bs"""
    return (np.repeat(agg.astype(np.int64), bs) * bs + np.tile(np.arange(bs), agg.size))


# ---------------------------------------------------------------------------------------------------------------------
# setup identities

def check_partition(lev):
    agg, nc, bs = lev["agg"], lev["coarse_cells"], lev["block_size"]
    assert agg.shape == (lev["n"] // bs,)
    assert agg.min() == 0 and agg.max() == nc - 1
    sizes = np.bincount(agg, minlength=nc)
    assert sizes.min() >= 1  # no empty aggregate; every cell has exactly one coarse cell by construction of the map
    if lev["mptr"] is not None:
        assert np.array_equal(lev["mptr"], np.concatenate([[0], np.cumsum(sizes)]))
        assert np.array_equal(lev["mem"], np.argsort(agg, kind="stable"))  # members ascending per coarse cell
    return sizes


def galerkin_reference(A, agg, bs, dtype, reverse=False):
    """P^T A P with sorted, summed duplicates; also the sum of the absolute contributions of every coarse row."""
    um = unknown_map(agg, bs)
    row = row_of_entries(A)
    R, Cc, v = um[row], um[A.indices], A.data.astype(dtype)
    if reverse:
        R, Cc, v = R[::-1], Cc[::-1], v[::-1]
    nc = int(agg.max() + 1) * bs
    order = np.lexsort((Cc, R))  # stable: duplicates stay in stored order
    R, Cc, v = R[order], Cc[order], v[order]
    head = np.concatenate([[True], (R[1:] != R[:-1]) | (Cc[1:] != Cc[:-1])])
    starts = np.flatnonzero(head)
    vals = np.add.reduceat(v, starts)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(R[starts], minlength=nc))]).astype(np.int64)
    rowabs = np.bincount(R, weights=np.abs(v).astype(np.float64), minlength=nc)
    return indptr, Cc[starts], vals, rowabs


def check_galerkin(lev, nxt, mutate=None):
    """A_{l+1} = P^T A_l P, entry by entry, with A_l the matrix the code coarsened (the read-out "A")."""
    A = lev["A"] if mutate is None else mutate(lev["A"])
    ip, ix, ref, rowabs = galerkin_reference(A, lev["agg"], lev["block_size"], LD)
    _, _, alt, _ = galerkin_reference(A, lev["agg"], lev["block_size"], np.float64, reverse=True)
    An = nxt["A"]
    assert np.array_equal(An.indptr, ip), "pattern of the coarse matrix (row lengths)"
    assert np.array_equal(An.indices, ix), "pattern of the coarse matrix (columns, ascending)"
    scale = rowabs[row_of_entries(An)]
    assert scale.min() > 0
    base = float(np.max(np.abs(alt.astype(LD) - ref) / scale))
    bound = FACTOR * max(base, EPS / 8)  # (a row of one or two contributions is exact in both evaluations)
    err = float(np.max(np.abs(An.data.astype(LD) - ref) / scale))
    assert bound <= HARD
    assert err <= bound, ("Galerkin", err, bound)
    return base, bound, err


def filter_reference(S, bs, theta, dtype, reverse=False):
    """The strength filter of amg.inc (amg_filter) on the host: block (i, j) is dropped when its strength -- the sum of the
    absolute diagonal entries of the bs x bs block -- is below theta * min(max_k s_ik, max_k s_jk) over the off-diagonal
    blocks; a dropped block is added to the diagonal block of its row, component by component."""
    n = S.shape[0]
    ip, ix, val = S.indptr.astype(np.int64), S.indices, S.data
    ent_row = row_of_entries(S)
    ent_off = np.arange(S.nnz) - ip[ent_row]
    ent_kb, ent_b = ent_off // bs, ent_off % bs
    cell = ent_row // bs
    first = ent_b == 0  # one representative entry per (row, block)
    rb_row, rb_kb, rb_cell = ent_row[first], ent_kb[first], cell[first]
    rb_cj = ix[ip[rb_row] + rb_kb * bs] // bs
    s = np.zeros(rb_row.size)
    for a in range(bs):  # in the order the kernel adds them
        s = s + np.abs(val[ip[rb_cell * bs + a] + rb_kb * bs + a])
    rmax = np.zeros(n // bs)
    off = rb_cj != rb_cell
    np.maximum.at(rmax, rb_cell[off], s[off])
    keep_rb = (~off) | (s >= theta * np.minimum(rmax[rb_cell], rmax[rb_cj]))
    rb_id = np.cumsum(first) - 1
    keep = keep_rb[rb_id]
    isdiag = (~off)[rb_id]
    assert np.all(np.bincount(rb_row[~off], minlength=n) == 1), "one diagonal block per row"
    f_ip = np.concatenate([[0], np.cumsum(np.bincount(ent_row[keep], minlength=n))])
    f_ix = ix[keep]
    f_val = val[keep].astype(dtype)
    # dropped mass per (row, component)
    dk = ent_row[~keep] * bs + ent_b[~keep]
    dv = val[~keep].astype(dtype)
    if reverse:
        dk, dv = dk[::-1], dv[::-1]
    lump = np.zeros(n * bs, dtype=dtype)
    if dk.size:
        o = np.argsort(dk, kind="stable")
        dk, dv = dk[o], dv[o]
        st = np.flatnonzero(np.concatenate([[True], dk[1:] != dk[:-1]]))
        lump[dk[st]] = np.add.reduceat(dv, st)
    dpos = np.flatnonzero((isdiag & keep)[keep])  # positions of the diagonal blocks' entries in the filtered arrays
    drow, db = ent_row[keep][dpos], ent_b[keep][dpos]
    f_val[dpos] = f_val[dpos] + lump[drow * bs + db]
    rowabs = np.bincount(ent_row, weights=np.abs(val), minlength=n)
    return f_ip, f_ix, f_val, rowabs, int((~keep).sum())


def check_filter(lev0):
    """The read-out matrix level 0 was coarsened from is the host-filtered system: pattern exactly, values to rounding."""
    S, F, bs, theta = lev0["sys"], lev0["A"], lev0["block_size"], lev0["filter_theta"]
    if theta == 0.0:
        assert np.array_equal(F.indptr, S.indptr) and np.array_equal(F.indices, S.indices)
        assert np.array_equal(F.data, S.data)
        return 0.0, 0.0, 0.0, 0
    ip, ix, ref, rowabs, dropped = filter_reference(S, bs, theta, LD)
    _, _, alt, _, _ = filter_reference(S, bs, theta, np.float64, reverse=True)
    assert np.array_equal(F.indptr, ip), "filtered pattern (row lengths)"
    assert np.array_equal(F.indices, ix), "filtered pattern (columns, kept in stored order)"
    scale = rowabs[row_of_entries(F)]
    base = float(np.max(np.abs(alt.astype(LD) - ref) / scale))
    bound = FACTOR * max(base, EPS / 8)
    err = float(np.max(np.abs(F.data.astype(LD) - ref) / scale))
    assert bound <= HARD and err <= bound, ("filter", err, bound)
    return base, bound, err, dropped


def check_dinv(lev, safe_rows, smooths):
    """dinv = 1 / a_ii of the operator the cycle reads, with the row safeguard (amg_safeguard_rows) on smoothed levels:
    rows with r = sum_{j != i} |a_ij| / |a_ii| > 1 get 2 / (a_ii (1 + r)).  A row sum of m terms in any order and four
    more operations: (m + 8) eps relative."""
    M = lev["op"]
    row = row_of_entries(M)
    isd = M.indices == row
    v = M.data.astype(LD)
    n = M.shape[0]
    d = np.zeros(n, dtype=LD)
    np.add.at(d, row[isd], v[isd])
    offs = np.zeros(n, dtype=LD)
    np.add.at(offs, row[~isd], np.abs(v[~isd]))
    ref = np.where(d != 0, 1 / np.where(d != 0, d, 1), 0)
    if safe_rows and smooths:
        r = offs * np.abs(ref)
        ref = np.where(r > 1, ref * 2 / (1 + r), ref)
    tol = (np.diff(M.indptr) + 8) * EPS
    err = np.abs(lev["dinv"].astype(LD) - ref) / np.maximum(np.abs(ref), np.finfo(np.float64).tiny)
    assert np.all(err <= tol), ("dinv", float(err.max()))


def check_dense(lev):
    """inverse times A_L = I, judged against what numpy.linalg.inv leaves on the same matrix."""
    A = lev["A"]
    n = A.shape[0]
    At = sps.csr_matrix(A.T).astype(LD)
    res = lambda inv: float(np.abs((At @ inv.T.astype(LD)).T - np.eye(n)).sum(axis=1).max())
    base = res(np.linalg.inv(A.toarray()))
    err = res(lev["dense"])
    assert err <= FACTOR * base, ("dense inverse", err, base)
    return base, err


def check_setup(H, safe_rows=None, galerkin_mutate=None):
    """All setup identities of one read-out hierarchy; returns the figures."""
    bs = H[0]["block_size"]
    safe_rows = (bs == 1) if safe_rows is None else safe_rows
    out = {"levels": len(H), "rows": [h["n"] for h in H], "galerkin": [], "filter": check_filter(H[0])}
    assert all(h["levels"] == len(H) for h in H)
    for l, lev in enumerate(H):
        last = l + 1 == len(H)
        assert lev["A"].shape == (lev["n"], lev["n"]) and lev["n"] % bs == 0
        if l == 0:
            src = lev["A"] if lev["filter_level0"] else lev["sys"]
        else:
            src = lev["A"]
        # the operator of the cycle is the matrix the code says it is, bit for bit
        assert np.array_equal(lev["op"].indptr, src.indptr) and np.array_equal(lev["op"].indices, src.indices)
        assert np.array_equal(lev["op"].data, src.data)
        check_dinv(lev, safe_rows, smooths=(not last) or (not lev["dense_ok"]))
        if last:
            assert lev["agg"] is None and lev["coarse_cells"] == 0
            if lev["dense_ok"]:
                assert lev["n"] <= lev["dense_max"] and "dense" in lev["path"]
                out["dense"] = check_dense(lev)
            else:
                assert "jacobi" in lev["path"] and lev["dense"] is None
            continue
        check_partition(lev)
        assert H[l + 1]["n"] == lev["coarse_cells"] * bs
        out["galerkin"].append(check_galerkin(lev, H[l + 1], galerkin_mutate if l == 0 else None))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cycle, from the header comment of amg.inc

class RefCycle:
    """One (1,1) cycle: damped Jacobi from zero, restriction by member sums, coarse correction scaled by alpha, the
    levels gamma / gamma_levels select visited a second time on the residual, damped Jacobi; coarsest level by the
    read-out inverse or by the Jacobi fallback (first step from zero, then two sweeps of two steps).  Only read-out data;
    matrix values rounded to FP32 where the library reads FP32."""

    def __init__(self, H, dtype=LD, reverse=False, skip_second=False):
        self.H, self.dtype, self.skip_second = H, dtype, skip_second
        self.nlev = len(H)
        self.A, self.Pt, self.um = [], [], []
        for l, lev in enumerate(H):
            M = lev["op"]
            data = M.data.astype(np.float32).astype(np.float64) if lev["fp32"] else M.data
            M = sps.csr_matrix((data, M.indices, M.indptr), shape=M.shape)
            if reverse:
                M = reversed_rows(M)
            self.A.append(sps.csr_matrix((M.data.astype(dtype), M.indices, M.indptr), shape=M.shape))
            if l + 1 < self.nlev:
                um = unknown_map(lev["agg"], lev["block_size"])
                nc = lev["coarse_cells"] * lev["block_size"]
                Pt = sps.csr_matrix((np.ones(um.size), (um, np.arange(um.size))), shape=(nc, um.size))
                Pt.sort_indices()  # members ascending
                if reverse:
                    Pt = reversed_rows(Pt)
                self.Pt.append(sps.csr_matrix((Pt.data.astype(dtype), Pt.indices, Pt.indptr), shape=Pt.shape))
                self.um.append(um)
        self.dinv = [lev["dinv"].astype(dtype) for lev in H]
        self.omega = [dtype(lev["omega"]) for lev in H]
        self.alpha = dtype(H[0]["alpha"])
        self.gamma, self.gamma_levels = H[0]["gamma"], H[0]["gamma_levels"]
        self.dense = None if H[-1]["dense"] is None else H[-1]["dense"].astype(dtype)
        self.second_visits = 0

    def smooth(self, l, x, b):
        return x + self.omega[l] * self.dinv[l] * (b - self.A[l] @ x)

    def cycle(self, l, b):
        if l + 1 == self.nlev:
            if self.dense is not None:
                return self.dense @ b
            x = self.omega[l] * self.dinv[l] * b
            for _ in range(4):
                x = self.smooth(l, x, b)
            return x
        x = self.omega[l] * self.dinv[l] * b
        bc = self.Pt[l] @ (b - self.A[l] @ x)
        xc = self.cycle(l + 1, bc)
        if self.gamma == 2 and l < self.gamma_levels and l + 2 < self.nlev and not self.skip_second:
            self.second_visits += 1
            xc = xc + self.cycle(l + 1, bc - self.A[l + 1] @ xc)
        t = x + self.alpha * xc[self.um[l]]
        return self.smooth(l, t, b)

    def __call__(self, R):
        return np.array([self.cycle(0, np.asarray(r, dtype=self.dtype)) for r in np.atleast_2d(R)])


def case_vectors(H, seed=0, n_unit=16):
    """Random vectors, the constant, a vector spanning 1e-8 .. 1e8, and unit vectors: last row block, a singleton
    aggregate when there is one (else a smallest one), the largest aggregate, and n_unit random ones."""
    n, bs = H[0]["n"], H[0]["block_size"]
    rng = np.random.default_rng(seed)
    vec = [rng.standard_normal(n) for _ in range(3)] + [np.ones(n)]
    vec.append(rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n))
    units = [n - 1 - int(rng.integers(0, min(n, 64) if n % 64 == 0 else n % 64))]
    if H[0]["agg"] is not None:
        sizes = np.bincount(H[0]["agg"])
        units.append(int(np.flatnonzero(H[0]["agg"] == np.argmin(sizes))[0]) * bs)
        units.append(int(np.flatnonzero(H[0]["agg"] == np.argmax(sizes))[-1]) * bs + bs - 1)
    units += [int(i) for i in rng.choice(n, min(n_unit, n), replace=False)]
    for i in units:
        e = np.zeros(n)
        e[i] = 1.0
        vec.append(e)
    return np.array(vec)


def max_rel(Z, Zref):
    Z, Zref = np.atleast_2d(Z), np.atleast_2d(Zref)
    scale = np.abs(Zref).max(axis=1)
    assert np.all(scale > 0)
    return float(np.max(np.abs(Z.astype(LD) - Zref).max(axis=1) / scale))


def check_cycle(ctx, lib, H, seed=0, dtype=LD, mutate_H=None, skip_second=False, V=None):
    """The library's cycle against the reference on the vectors of the case; returns baseline, bound and error."""
    V = case_vectors(H, seed) if V is None else V
    Z = apply_cycle(ctx, lib, V)
    Hm = H if mutate_H is None else mutate_H(H)
    ref = RefCycle(Hm, dtype, skip_second=skip_second)
    Zref = ref(V)
    Zalt = RefCycle(Hm, np.float64, reverse=True, skip_second=skip_second)(V)
    base = max_rel(Zalt, Zref)
    bound = FACTOR * base
    err = max_rel(Z, Zref)
    assert 0 < bound <= HARD, ("the case is ill-conditioned for the purpose", bound)
    assert err <= bound, ("cycle", err, bound)
    if H[0]["gamma"] == 2 and not skip_second:
        want = sum(1 for l in range(len(H)) if "second_visit" in H[l]["path"])
        assert (ref.second_visits > 0) == (want > 0)
    # linearity at rounding level, and two applies are the same bits
    a, b = 0.75, -1.5
    lin = apply_cycle(ctx, lib, a * V[0] + b * V[1])[0]
    lerr = max_rel(lin, (a * Z[0].astype(LD) + b * Z[1].astype(LD))[None, :])
    assert lerr <= bound, ("linearity", lerr, bound)
    assert np.array_equal(apply_cycle(ctx, lib, V[:3]), Z[:3]), "two applies differ"
    return {"baseline": base, "bound": bound, "error": err, "vectors": V, "Z": Z}


def paths(H):
    return [sorted(h["path"]) for h in H]


def run_case(sysm, lib, n_own=0, env=None, seed=0, expect=None):
    """Setup under `env`, read-out, all identities and the cycle; `expect(H)` asserts the path the case is for."""
    with environment(env or {}):
        sysm.ctx.amg_setup(n_own)
        H = read_hierarchy(sysm.ctx)
        out = check_setup(H)
        if expect is not None:
            expect(H)
        out["cycle"] = check_cycle(sysm.ctx, lib, H, seed)
    out["H"] = H
    out["paths"] = paths(H)
    return out


def hierarchies_equal(Ha, Hb, tol):
    """Launch-only switches: maps bitwise, patterns bitwise, values to `tol` relative to the largest entry of the row."""
    assert len(Ha) == len(Hb)
    for a, b in zip(Ha, Hb):
        for k in ("agg", "mptr", "mem"):
            assert (a[k] is None) == (b[k] is None) and (a[k] is None or np.array_equal(a[k], b[k])), k
        for k in ("A", "op"):
            assert np.array_equal(a[k].indptr, b[k].indptr) and np.array_equal(a[k].indices, b[k].indices), k
            scale = np.maximum.reduceat(np.abs(a[k].data), a[k].indptr[:-1])[row_of_entries(a[k])]  # (no empty rows)
            assert np.all(np.abs(a[k].data - b[k].data) <= tol * scale), k
        assert np.all(np.abs(a["dinv"] - b["dinv"]) <= tol * np.abs(a["dinv"]))
        assert a["omega"] == b["omega"] and a["alpha"] == b["alpha"]


def switch_matrix(make_system, lib, extra=None, expect_default=None):
    """Every variant against its own read-out reference; a variant that only changes how the work is launched is also
    compared with the variant it must equal: read-out hierarchies (maps bitwise, values to rounding) and applied vectors."""
    sysm = make_system()
    sysm.ctx.amg_setup(0)
    bs = sysm.ctx.amg_level(0)["block_size"]
    lanes = "0" if bs == 1 else "1"  # (the default is on for scalar systems only)
    g2 = {"PFV_AMG_GAMMA": "2"}
    # name -> (switches, the variant it must equal or None)
    variants = {
        "default": ({}, None),
        "fuse_cycle=0": ({"PFV_AMG_FUSE_CYCLE": "0"}, "default"),
        "gamma=2": (g2, None),
        "gamma=2,levels=2": (dict(g2, PFV_AMG_GAMMA_LEVELS="2"), None),
        "fuse_rows=0,gamma=2": (dict(g2, PFV_AMG_FUSE_ROWS="0"), "gamma=2"),
        "fuse_rows=0,gamma=2,fuse_cycle=0": (dict(g2, PFV_AMG_FUSE_ROWS="0", PFV_AMG_FUSE_CYCLE="0"), "gamma=2"),
        "window=0": ({"PFV_SPMV_WINDOW": "0"}, "default"),
        "fp32=0": ({"PFV_AMG_FP32": "0"}, None),
        "restrict_lanes flipped": ({"PFV_AMG_RESTRICT_LANES": lanes}, "default"),
        "galerkin_batched=0": ({"PFV_AMG_GALERKIN_BATCHED": "0"}, "default"),
    }
    results = {}
    V = None
    for name, (env, _) in variants.items():
        full = dict(extra or {}, PFV_AMG_REUSE="0")  # every variant matches afresh
        full.update(env)
        with environment(full):
            sysm.ctx.amg_setup(0)
            H = read_hierarchy(sysm.ctx)
            res = check_setup(H)
            V = case_vectors(H, 3) if V is None else V
            res["cycle"] = check_cycle(sysm.ctx, lib, H, V=V)
        res["H"], res["paths"] = H, paths(H)
        results[name] = res
        every = set().union(*[h["path"] for h in H])
        if name == "default" and expect_default is not None:
            expect_default(H)
        if "gamma=2" in name:
            assert "second_visit" in every and H[0]["gamma"] == 2, name
            assert ("second_visit_fused" in every) == ("fuse_cycle=0" not in name), name
        if "levels=2" in name and len(H) >= 4:
            assert "second_visit" in H[0]["path"] and "second_visit" in H[1]["path"], name
        if "fuse_cycle=0" in name:
            assert not ({"fused_product", "second_visit_fused"} & every), name
        if "fuse_rows=0" in name:
            assert not ({"restrict_residual", "prolong_smooth"} & every), name
            if "fuse_cycle=0" not in name:
                assert all("fused_product" in h["path"] for h in H[1:-1]), name
        if name == "fp32=0":
            assert not any(h["fp32"] for h in H)
        else:
            assert all(h["fp32"] for h in H)
        if name == "window=0":
            assert not any(h["window"] for h in H)
        if name.startswith("restrict_lanes"):
            assert H[0]["restrict_lanes"] != results["default"]["H"][0]["restrict_lanes"]
    for name, (_, same_as) in variants.items():
        if same_as is None:
            continue
        a, b = results[same_as], results[name]
        tol = max(a["cycle"]["bound"], b["cycle"]["bound"])
        hierarchies_equal(a["H"], b["H"], tol)
        assert max_rel(b["cycle"]["Z"], a["cycle"]["Z"].astype(LD)) <= tol, name
    return results


# ---------------------------------------------------------------------------------------------------------------------
# state: what a re-setup keeps

def state_sequence(lib, n=8):
    """One handle, a sequence of setups, read-out and identities after each."""
    g = tet_grid(n)
    S = FlowSystem(lib, g, seed=4, sigma=0.5)
    rng = np.random.default_rng(9)
    log = []

    def step(tag, reused, env=None):
        res = run_case(S, lib, env=env, seed=len(log))
        assert res["H"][0]["reused"] == reused, (tag, res["H"][0]["reused"])
        assert abs(res["H"][0]["sys"] - S.A).max() == 0.0, tag  # the hierarchy belongs to the values on the handle NOW
        log.append((tag, res))
        return res

    first = step("first", False)
    sc1 = S.sc
    # same values, three setups: the third is offered the kept filter layout
    step("same values 2", True)
    step("same values 3", True)
    assert S.ctx.stats()["amg_maps_reused"] == 1
    assert S.ctx.stats()["amg_filter_layout"] == 1  # (wrote into the kept layout -- and the filtered operator is right)
    # new values, same pattern: the values-only branch, and every level satisfies the identities for the NEW values
    S.set_values(sc1 * np.exp(0.1 * rng.standard_normal(g.num_cells)))
    moved = step("new values", True)
    assert S.ctx.stats()["amg_filter_layout"] == 2  # (the kept layout was tried, did not fit, and the filter was redone)
    assert len(moved["H"]) == len(first["H"])
    for a, b in zip(first["H"][:-1], moved["H"][:-1]):
        assert np.array_equal(a["agg"], b["agg"])  # kept maps
    assert not np.array_equal(first["H"][1]["A"].data, moved["H"][1]["A"].data)
    # the mutation this guards against: the previous values' level matrix fed to the Galerkin check must fail
    stale = first["H"][0]["A"]
    try:
        check_galerkin(dict(moved["H"][0], A=stale), moved["H"][1])
    except AssertionError:
        pass
    else:
        raise AssertionError("a stale level matrix passes the Galerkin check")
    # control: PFV_AMG_REUSE=0 matches afresh on the same values
    ctrl = step("control", False, env={"PFV_AMG_REUSE": "0"})
    assert np.array_equal(ctrl["H"][0]["A"].data, moved["H"][0]["A"].data)
    step("rematch after the control", False)  # (a setup with PFV_AMG_REUSE=0 leaves no maps behind)
    # values under which the filter keeps other entries (strong heterogeneity): the filtered operator is recomputed
    S.set_values(sc1 * np.exp(1.5 * rng.standard_normal(g.num_cells)))
    with environment({"PFV_AMG_REUSE": "1"}):
        het = step("filter moves", True)
    assert not np.array_equal(het["H"][0]["A"].indptr, moved["H"][0]["A"].indptr), "the filter kept the same entries"
    # a rebuilt topology that the digest proves unchanged, then new permeabilities
    S.set_values(S.sc, rebuild=True)
    step("rebuilt topology", True)
    S.set_values(sc1 * np.exp(0.2 * rng.standard_normal(g.num_cells)), rebuild=True)
    step("rebuilt topology, new values", True)
    return log


def matching_switch_change_rematches(lib, n=8):
    """A switch the matching depends on invalidates the kept maps, both when it is set and when it is removed again:
    the setup after the change re-matches, and its maps are those of a fresh handle under the same switches."""
    g = tet_grid(n)
    S = FlowSystem(lib, g, seed=4)

    def setup(sysm, reused, env=None):
        with environment(env or {}):
            sysm.ctx.amg_setup(0)
            H = read_hierarchy(sysm.ctx)
            assert H[0]["reused"] == reused, (env, H[0]["reused"])
            check_setup(H)
        return H

    def same_maps(Ha, Hb):
        assert len(Ha) == len(Hb)
        for a, b in zip(Ha, Hb):
            for k in ("agg", "mptr", "mem"):
                assert (a[k] is None) == (b[k] is None) and (a[k] is None or np.array_equal(a[k], b[k])), k

    first = setup(S, False)
    assert len(first) >= 3
    same_maps(setup(S, True), first)
    for env in ({"PFV_AMG_ROUNDS": "1"}, {"PFV_AMG_STRENGTH_NEG": "1"}, {"PFV_AMG_PASSES_COARSE": "1"}):
        same_maps(setup(S, False, env), setup(FlowSystem(lib, g, seed=4), False, env))
        same_maps(setup(S, False), first)
    return len(first)


def different_pattern_same_sizes(lib, n=900, seed=12):
    """Two user systems with equal rows and nnz but different patterns on one handle: the maps must be rebuilt."""
    rng = np.random.default_rng(seed)
    A = graph_matrix(n, rng)
    A.sort_indices()
    perm = rng.permutation(n)
    B = sps.csr_matrix(A[perm][:, perm])
    assert B.nnz == A.nnz and B.shape == A.shape and not np.array_equal(A.indices, B.indices)
    S = UserSystem(lib, A)
    r1 = run_case(S, lib)
    S.A = B
    S.ctx.set_system(B, S.b)
    r2 = run_case(S, lib)
    assert not r2["H"][0]["reused"]
    S.ctx.set_system(B, S.b)
    r3 = run_case(S, lib)
    assert r3["H"][0]["reused"]
    return r1, r2, r3


def leading_block(lib, n=1400, n_own=1000, seed=21):
    """pfv_amg_setup(n_own) with n_own < n: the hierarchy of the leading block extracted on the host."""
    rng = np.random.default_rng(seed)
    A = shuffled_columns(graph_matrix(n, rng), rng)
    S = UserSystem(lib, A)
    S.ctx.amg_setup(n_own)
    H = read_hierarchy(S.ctx)
    assert H[0]["n"] == n_own
    row = row_of_entries(A)
    keep = (row < n_own) & (A.indices < n_own)
    ip = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=n)[:n_own])])
    assert np.array_equal(H[0]["sys"].indptr, ip)
    assert np.array_equal(H[0]["sys"].indices, A.indices[keep]) and np.array_equal(H[0]["sys"].data, A.data[keep])
    out = check_setup(H)
    out["cycle"] = check_cycle(S.ctx, lib, H, seed=2)
    # ... and it is the hierarchy a handle gets that is given the block alone
    T = UserSystem(lib, sps.csr_matrix((A.data[keep], A.indices[keep], ip), shape=(n_own, n_own)))
    T.ctx.amg_setup(0)
    hierarchies_equal(H, read_hierarchy(T.ctx), 0.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the tests bite: mutations of the reference's inputs

def expect_failure(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError("mutation not detected: " + what)


def mutations(lib, n=10):
    """Each mutation of the reference side must make the corresponding check fail (the library is left alone)."""
    S = FlowSystem(lib, tet_grid(n), seed=6)
    # (PFV_AMG_OMEGA_AUTO: every level gets its own damping from the power iteration -- something to swap)
    with environment({"PFV_AMG_GAMMA": "2", "PFV_AMG_REUSE": "0", "PFV_AMG_OMEGA_AUTO": "1"}):
        S.ctx.amg_setup(0)
        H = read_hierarchy(S.ctx)
        assert len(H) >= 3
        check_setup(H)
        V = case_vectors(H, 1)
        check_cycle(S.ctx, lib, H, V=V)

        def scaled_entry(Hh):
            Hm = [dict(h) for h in Hh]
            M = Hm[1]["op"].copy()
            M.data = M.data.copy()
            k = M.nnz // 2
            M.data[k] *= 1 + 1e-8 * 4096  # (beyond the FP32 rounding the cycle reads the values with)
            Hm[1]["op"] = M
            return Hm

        def scaled_entry_galerkin():
            nxt = dict(H[1])
            M = nxt["A"].copy()
            M.data = M.data.copy()
            M.data[M.nnz // 2] *= 1 + 1e-8
            nxt["A"] = M
            check_galerkin(H[0], nxt)

        def swapped_omegas(Hh):
            Hm = [dict(h) for h in Hh]
            assert abs(Hh[0]["omega"] - Hh[1]["omega"]) > 1e-3
            Hm[0]["omega"], Hm[1]["omega"] = Hh[1]["omega"], Hh[0]["omega"]
            return Hm

        def moved_cell(Hh):
            Hm = [dict(h) for h in Hh]
            agg = Hm[0]["agg"].copy()
            i = agg.size // 2
            nb = Hh[0]["A"].indices[Hh[0]["A"].indptr[i]:Hh[0]["A"].indptr[i + 1]]
            other = [a for a in agg[nb] if a != agg[i]]
            agg[i] = other[0]
            Hm[0]["agg"] = agg
            return Hm

        expect_failure(scaled_entry_galerkin, "one coarse entry scaled by 1 + 1e-8 (Galerkin)")
        expect_failure(lambda: check_cycle(S.ctx, lib, H, V=V, mutate_H=scaled_entry), "one coarse entry scaled (cycle)")
        expect_failure(lambda: check_cycle(S.ctx, lib, H, V=V, mutate_H=swapped_omegas), "omegas of two levels swapped")
        expect_failure(lambda: check_cycle(S.ctx, lib, H, V=V, mutate_H=moved_cell), "one cell moved (cycle)")
        expect_failure(lambda: check_galerkin(moved_cell(H)[0], H[1]), "one cell moved (Galerkin)")
        expect_failure(lambda: check_cycle(S.ctx, lib, H, V=V, skip_second=True), "second visit left out")
    return True
