"""Interaction regions of an exact size: grids, problems and checks shared by tests/test_node_class_emulation.py (host
emulation) and tests/test_gpu_node_class.py (product library).

The node kernels pick their body by the number n of faces that meet in a node (csrc/ctx.h: kClassBounds; csrc/
mpfa_numeric.inc: launch_node_kernel; csrc/mpsa.inc: mpsa_node_body).  ``fan_grid_3d(n)`` builds a grid whose hub and
pole are met by exactly n faces, so that every class edge, the unpivoted elimination's classes and its redo hand-over can
be reached on purpose.  Every input here is a regular, well-conditioned problem; the redo path is reached through the
acceptance tolerance (PFV_NODE_NP_TOLX / PFV_MPSA_NP_TOLX = 0), never through an input that breaks an elimination."""
from __future__ import annotations

import numpy as np

import porepy_amd as pa
from oracle import mpfa_oracle as mo
from oracle import mpsa_oracle as so
from tests._golden import ALL_KEYS, MPSA_KEYS, rel_max_err
from tests._parity import MPSA_WHICH, TOL, WHICH

# faces per node at which the MPFA launcher changes the instantiation (8 | 16 | 32 | <64,40> | <64,48> | <64,64> | LDS),
# the rows per lane (NR + 7) / 8 or the class (kClassBounds), one value on either side of each edge
MPFA_EDGES = (5, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 64, 65, 96, 97)
# MPSA: the class edges, 42 | 43 = the register elimination's nd n <= 128 (126 against 129 unknowns), 129 = the largest
MPSA_EDGES = (5, 8, 9, 16, 17, 32, 33, 40, 41, 42, 43, 48, 49, 64, 65, 129)
ENV_SWITCHES = ("PFV_NODE_GJ", "PFV_NODE_NP_TOLX", "PFV_MPSA_GJ_NP", "PFV_MPSA_NP_TOLX", "PFV_MPSA_REDO_WIDE")


# ------------------------------------------------------------------------------------------------------ grids
def _fan_points_tets(n: int):
    """Points (3, m + 2) and tetrahedra (hub 0, pole 1, ring_i, ring_i+1) of the fan with n faces at hub and pole:
    closed ring of m = n / 2 points for even n, open fan over 1.5 pi of m = (n + 1) / 2 points for odd n."""
    if n < 5:
        raise ValueError("fan_grid_3d: n >= 5")
    closed = n % 2 == 0
    m = n // 2 if closed else (n + 1) // 2
    step = 2.0 * np.pi / m if closed else 1.5 * np.pi / (m - 1)
    rng = np.random.default_rng(7000 + n)
    # in-plane jitter: about 0.05 radially, along the ring at most a quarter of the spacing (neighbours never swap)
    radius = 1.0 + 0.05 * (2.0 * rng.random(m) - 1.0)
    angle = step * np.arange(m) + min(0.05, 0.25 * step) * (2.0 * rng.random(m) - 1.0)
    ring = np.vstack((radius * np.cos(angle), radius * np.sin(angle), np.zeros(m)))
    pts = np.hstack((np.zeros((3, 1)), np.array([[0.02], [0.03], [0.8]]), ring))
    i = np.arange(m if closed else m - 1)
    tets = np.stack((np.zeros_like(i), np.ones_like(i), 2 + i, 2 + (i + 1) % m), axis=1)
    # every tetrahedron positively oriented (pole above the plane, ring counter-clockwise): no overlap, no inversion
    vol = np.einsum("ij,ij->j", pts[:, tets[:, 1]], np.cross(pts[:, tets[:, 2]], pts[:, tets[:, 3]], axis=0))
    assert np.all(vol > 1e-4), (n, vol.min())
    return pts, tets


def faces_per_node(g) -> np.ndarray:
    raw = pa.grid_to_raw(g)
    return np.bincount(raw["fn_indices"], minlength=g.num_nodes)


def fan_union_3d(ns):
    """Disjoint union of the fans of ``ns`` as ONE grid, the k-th shifted by (3 k, 0, 0): hubs of different classes in
    the same discretization.  ``g.fan_hubs[k]`` = (hub, pole) node ids, ``g.fan_cells[k]`` = cell ids of the k-th fan."""
    P, T, hubs, cells = [], [], [], []
    np_off = nc_off = 0
    for k, n in enumerate(ns):
        pts, tets = _fan_points_tets(n)
        P.append(pts + np.array([[3.0 * k], [0.0], [0.0]]))
        T.append(tets + np_off)
        hubs.append((np_off, np_off + 1))
        cells.append(np.arange(nc_off, nc_off + tets.shape[0]))
        np_off += pts.shape[1]
        nc_off += tets.shape[0]
    g = pa.TetrahedralGrid(np.hstack(P), np.vstack(T))
    g.compute_geometry()
    cnt = faces_per_node(g)
    for n, (hub, pole) in zip(ns, hubs):
        assert cnt[hub] == n and cnt[pole] == n, (n, cnt[hub], cnt[pole])
    ring = np.setdiff1d(np.arange(g.num_nodes), np.ravel(hubs))
    assert cnt[ring].max() <= 6  # (the ring nodes: a small class in every grid)
    g.fan_hubs, g.fan_cells = hubs, cells
    return g


def fan_grid_3d(n: int):
    """Tetrahedral fan whose hub (node 0, origin) and pole (node 1) are each met by exactly n faces (asserted)."""
    return fan_union_3d((n,))


def lattice_grid():
    g = pa.StructuredTetrahedralGrid([4, 4, 4], [1.0, 1.0, 1.0])
    g.compute_geometry()
    return g


def count_between(g, lo: int, hi: int, scale: int = 1) -> int:
    """Number of nodes with lo < scale * n <= hi."""
    c = scale * faces_per_node(g)
    return int(np.count_nonzero((c > lo) & (c <= hi)))


# --------------------------------------------------------------------------------------------------- problems
class Problem:
    """One grid with its parameters and, computed once and left alone, the FP64 oracle's matrices."""

    def __init__(self, kind, g, tensor, bc):
        self.kind, self.g, self.tensor, self.bc = kind, g, tensor, bc
        self.raw = pa.grid_to_raw(g)
        self.eta = mo.default_eta(self.raw["name"])
        self._ora = None

    @property
    def keys(self):
        return ALL_KEYS if self.kind == "mpfa" else MPSA_KEYS

    @property
    def oracle(self):
        if self._ora is None:
            if self.kind == "mpfa":
                self._ora = mo.discretize(self.raw, self.tensor, pa.bc_to_raw(self.bc), eta=self.eta)
            else:
                self._ora = so.discretize(self.raw, self.tensor, self.bc, eta=self.eta)
        return self._ora


def _mixed_kinds(nb: int, robin: bool):
    kinds = np.where(np.arange(nb) % 3 == 0, "dir", "neu").astype(object)
    if robin:
        kinds[1] = "rob"
    return list(kinds)


def mpfa_problem(g, seed: int = 12, bench_like: bool = False, perm=None) -> Problem:
    """Full-tensor anisotropic K (the field of mpfa_large_interaction_region; ``bench_like``: the benchmark's 100 : 1
    anisotropy times a log-normal factor), every third boundary face Dirichlet, one Robin, the rest Neumann."""
    rng = np.random.default_rng(seed)
    nc = g.num_cells
    if perm is not None:
        K = perm
    elif bench_like:
        s = np.exp(0.5 * rng.standard_normal(nc))
        K = pa.SecondOrderTensor(kxx=s, kyy=10 * s, kzz=0.1 * s, kxy=0.5 * s, kxz=0.05 * s, kyz=0.2 * s).values
    else:
        k = 1 + rng.random(nc)
        K = pa.SecondOrderTensor(kxx=k, kyy=2 * k, kzz=0.5 * k, kxy=0.2 * k, kxz=0.05 * k, kyz=0.1 * k).values
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, _mixed_kinds(bf.size, robin=True))
    bc.robin_weight = 0.7 + np.random.default_rng(seed + 1).random(g.num_faces)
    return Problem("mpfa", g, K, bc)


def mpsa_problem(g, seed: int = 8) -> Problem:
    """Random Lame pair per cell (mpsa_large_interaction_region); every third boundary face clamped, the rest Neumann."""
    rng = np.random.default_rng(seed)
    nc, nf, nd = g.num_cells, g.num_faces, g.dim
    C = pa.FourthOrderTensor(1 + rng.random(nc), 0.5 + rng.random(nc)).values
    bf = g.get_all_boundary_faces()
    is_dir = np.zeros((nd, nf), bool)
    is_neu = np.zeros((nd, nf), bool)
    is_neu[:, bf] = True
    is_dir[:, bf[::3]] = True
    is_neu[:, bf[::3]] = False
    return Problem("mpsa", g, C, {"is_dir": is_dir, "is_neu": is_neu})


_PROBLEMS: dict = {}


def problem(kind: str, name):
    """Problems by name, shared by the tests of one process (grid, parameters and oracle made once): ``name`` is a fan's n,
    a tuple of them (union), "lattice" (4^3 Kuhn lattice, benchmark-like field) or "tri45" (45 x 45 triangles, MPSA)."""
    key = (kind, name)
    if key not in _PROBLEMS:
        if name == "lattice":
            p = mpfa_problem(lattice_grid(), seed=2, bench_like=True)
        elif name == "tri45":
            g = pa.StructuredTriangleGrid([45, 45], [1.0, 1.0])
            g.compute_geometry()
            p = mpsa_problem(g)
        else:
            g = fan_union_3d(name) if isinstance(name, tuple) else fan_grid_3d(name)
            p = mpfa_problem(g) if kind == "mpfa" else mpsa_problem(g)
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


# ------------------------------------------------------------------------------------------------------- runs
def open_context(lib, p: Problem):
    ctx = pa.Context(0, lib)
    ctx.set_grid(p.raw)
    return ctx


def discretize(ctx, p: Problem, monkeypatch=None, env=None):
    """One discretization on ``ctx`` under the switches ``env`` (set around this call only: env_int reads them per call);
    returns ({key: csr}, node_redo)."""
    with (monkeypatch.context() if monkeypatch is not None else _NoPatch()) as mp:
        for k in ENV_SWITCHES:
            if mp is not None:
                mp.delenv(k, raising=False)
        for k, v in (env or {}).items():
            mp.setenv(k, str(v))
        if p.kind == "mpfa":
            ctx.set_params(p.tensor, pa.bc_flags(p.bc), p.bc.robin_weight, p.eta)
            ctx.discretize()
            mats = {k: ctx.matrix(WHICH[k]) for k in ALL_KEYS}
        else:
            ctx.mpsa_set_params(p.tensor, p.g.cell_volumes, p.bc["is_dir"], p.bc["is_neu"], p.eta)
            ctx.mpsa_discretize()
            mats = {k: ctx.matrix(MPSA_WHICH[k]) for k in MPSA_KEYS}
        redo = int(ctx.stats()["node_redo"])
    return {k: m.copy() for k, m in mats.items()}, redo


class _NoPatch:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def run(lib, p: Problem, monkeypatch=None, env=None):
    ctx = open_context(lib, p)
    try:
        return discretize(ctx, p, monkeypatch, env)
    finally:
        ctx.close()


def worst_error(p: Problem, mats) -> float:
    """Patterns index for index against the oracle; returns the largest relative error over the matrices."""
    worst = 0.0
    for k in p.keys:
        M, R = mats[k], p.oracle[k]
        assert M.shape == R.shape, k
        assert np.array_equal(M.indptr, R.indptr) and np.array_equal(M.indices, R.indices), k
        worst = max(worst, rel_max_err(M, R))
    return worst


def assert_oracle(p: Problem, mats, what=""):
    err = worst_error(p, mats)
    print(f"{p.kind} {what}: worst relative error {err:.2e}")
    assert err < TOL, (what, err)


def same_bits(a, b) -> bool:
    return all(np.array_equal(a[k].indptr, b[k].indptr) and np.array_equal(a[k].indices, b[k].indices) and
               a[k].data.tobytes() == b[k].data.tobytes() for k in a)


def check_against_oracle(lib, kind: str, name):
    """Default switches: every matrix within TOL of the FP64 oracle, patterns equal.  Returns node_redo."""
    p = problem(kind, name)
    mats, redo = run(lib, p)
    assert_oracle(p, mats, f"n={name}")
    return redo


def partial_update_through_redo(lib, monkeypatch, expect_redo: int):
    """update_discretization (the entry check_partial_case drives) on the 36 + 44 union with PFV_NODE_NP_TOLX=0: new
    permeability in the cells of the n = 44 fan only.  node_redo counts that fan's hubs alone, the other fan's rows keep
    their bits, and the updated matrices are those of a fresh discretization and of the oracle."""
    p = problem("mpfa", (36, 44))
    g = p.g
    cells = g.fan_cells[1]
    perm_new = p.tensor.copy()
    perm_new[:, :, cells] *= 1.0 + 0.5 * np.random.default_rng(3).random(cells.size)
    p_new = mpfa_problem(g, perm=perm_new)
    key = "flow"

    def tensor(v):
        return type("K", (), {"values": v})()

    def mats_of(data):
        return {k: data[pa.DISCRETIZATION_MATRICES][key][k].copy() for k in ALL_KEYS}

    with monkeypatch.context() as mp:
        for k in ENV_SWITCHES:
            mp.delenv(k, raising=False)
        data = pa.initialize_data({}, key, {"second_order_tensor": tensor(p.tensor), "bc": p.bc})
        d = pa.Mpfa(key, library=lib)
        d.discretize(g, data)
        before = mats_of(data)
        assert_oracle(p, before, "union before the update")
        data[pa.PARAMETERS][key]["second_order_tensor"] = tensor(perm_new)
        data["update_discretization"] = {"modified_cells": cells}
        mp.setenv("PFV_NODE_NP_TOLX", "0")
        d.update_discretization(g, data)
        redo = int(d.context(g).stats()["node_redo"])
        mp.delenv("PFV_NODE_NP_TOLX")
        after = mats_of(data)
        fresh = pa.initialize_data({}, key, {"second_order_tensor": tensor(perm_new), "bc": p.bc})
        pa.Mpfa(key, library=lib).discretize(g, fresh)
        fresh = mats_of(fresh)
    assert redo == expect_redo, redo
    _, touched = pa.active_indices(g, cells=cells)
    untouched = np.setdiff1d(np.arange(g.num_faces), touched)
    cf = g.cell_faces.tocsc()
    faces0 = np.unique(cf.indices[cf.indptr[g.fan_cells[0][0]]: cf.indptr[g.fan_cells[0][-1] + 1]])
    assert np.array_equal(untouched, faces0)  # (the two fans share nothing: exactly the other fan's faces)
    for k in ALL_KEYS:
        assert after[k][untouched].data.tobytes() == before[k][untouched].data.tobytes(), k
        assert np.array_equal(after[k][untouched].indices, before[k][untouched].indices), k
        assert rel_max_err(after[k][touched], fresh[k][touched]) < TOL, k
        assert rel_max_err(after[k], fresh[k]) < TOL, k
    assert_oracle(p_new, after, "union after the update")
