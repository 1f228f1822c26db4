"""Cases for the sub-cell topology rebuild (porepy_amd/csrc/topology.inc), shared by the host-emulation suite
(tests/test_topology_rebuild_emulation.py) and the device suite (tests/test_gpu_topology_rebuild.py).

Every case exports the integer arrays and scalars the rebuild leaves in the handle (Context.debug_topology) and compares
them three ways: the node-cooperative construction against the reference construction (PFV_TOPO_LEGACY=1) bit for bit,
both against a numpy construction written here (np.lexsort on (node, entry), np.unique), and the topology digest of the
two paths.

Not covered: an "inconsistent cell_faces / face_nodes pair" (PFV_ERR_ARGUMENT).  With every index in range the records
and the sub-face lists both come from face_nodes, so no input reaches that status; an index out of range makes the
reference construction read past its arrays, which no test may do on a device."""
from __future__ import annotations

import contextlib
import os

import numpy as np
import pytest

import porepy_amd as pa

CLASS_BOUNDS = np.array([4, 8, 12, 16, 24, 32, 40, 48, 64, 96, 128, 192, 255])
ARRAYS = [name for name, _ in pa._lib.Context.TOPOLOGY_ARRAYS]
SCALARS = [k for k in pa._lib.Context.TOPOLOGY_SCALARS if k != "topology_path"]  # (which construction ran)


@contextlib.contextmanager
def topo_path(legacy: bool):
    old = os.environ.get("PFV_TOPO_LEGACY")
    os.environ["PFV_TOPO_LEGACY"] = "1" if legacy else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["PFV_TOPO_LEGACY"]
        else:
            os.environ["PFV_TOPO_LEGACY"] = old


# ------------------------------------------------------------------------------------ grids
def _regular(kind: str, nx, perturb: bool = False) -> dict:
    cls = {"cart": pa.CartGrid, "tri": pa.StructuredTriangleGrid, "tet": pa.StructuredTetrahedralGrid}[kind]
    g = cls(list(nx), [1.0] * len(nx))
    if perturb:
        rng = np.random.default_rng(7)
        h = 0.2 / max(nx)
        inner = np.all((g.nodes[: g.dim] > 1e-9) & (g.nodes[: g.dim] < 1 - 1e-9), axis=0)
        g.nodes[: g.dim, inner] += h * (rng.random((g.dim, int(inner.sum()))) - 0.5)
    g.compute_geometry()
    raw = pa.grid_to_raw(g)
    raw["name"] = f"{kind}{'x'.join(map(str, nx))}{'_perturbed' if perturb else ''}"
    return raw


def fan_2d(k: int) -> dict:
    """k triangles around node 0 (hand-made arrays): the hub has k sub-faces (the spokes) and 2 k records."""
    ang = 2 * np.pi * np.arange(k) / k
    nodes = np.zeros((3, k + 1))
    nodes[0, 1:], nodes[1, 1:] = np.cos(ang), np.sin(ang)
    nxt = (np.arange(k) + 1) % k
    spokes = np.stack((np.zeros(k, int), 1 + np.arange(k)), 1)  # faces 0 .. k-1
    rim = np.sort(np.stack((1 + np.arange(k), 1 + nxt), 1), axis=1)  # faces k .. 2k-1
    faces = np.vstack((spokes, rim))
    cell_faces = np.sort(np.stack((np.arange(k), nxt, k + np.arange(k)), 1), axis=1)
    pa_, pb_ = nodes[:, faces[:, 0]], nodes[:, faces[:, 1]]
    fc = 0.5 * (pa_ + pb_)
    t = pb_ - pa_
    fnorm = np.stack((t[1], -t[0], np.zeros(2 * k)))
    cc = (nodes[:, 0:1] + nodes[:, 1 + np.arange(k)] + nodes[:, 1 + nxt]) / 3.0
    sign = np.empty((k, 3), np.int8)
    for j in range(3):
        f = cell_faces[:, j]
        sign[:, j] = np.where(np.einsum("ij,ij->j", fnorm[:, f], fc[:, f] - cc) > 0, 1, -1)
    return {"dim": 2, "name": f"fan{k}", "nodes": nodes, "face_normals": fnorm, "face_centers": fc,
            "cell_centers": cc, "face_areas": np.linalg.norm(t, axis=0),
            "cell_volumes": np.full(k, 0.5 * np.sin(2 * np.pi / k)),
            "cf_indptr": 3 * np.arange(k + 1), "cf_indices": cell_faces.ravel(), "cf_sign": sign.ravel(),
            "fn_indptr": 2 * np.arange(2 * k + 1), "fn_indices": faces.ravel()}


def pyramid() -> dict:
    """One pyramid: four faces of the cell meet in its apex (node 4), not nd = 3."""
    nodes = np.array([[0, 1, 1, 0, 0.5], [0, 0, 1, 1, 0.5], [0, 0, 0, 0, 1.0]], float)
    faces = [[0, 1, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4], [0, 3, 4]]
    fc = np.stack([nodes[:, f].mean(axis=1) for f in faces], 1)
    cc = nodes.mean(axis=1, keepdims=True)
    fnorm = fc - cc
    return {"dim": 3, "name": "pyramid", "nodes": nodes, "face_normals": fnorm, "face_centers": fc, "cell_centers": cc,
            "face_areas": np.linalg.norm(fnorm, axis=0), "cell_volumes": np.array([1.0 / 3.0]),
            "cf_indptr": np.array([0, 5]), "cf_indices": np.arange(5), "cf_sign": np.ones(5, np.int8),
            "fn_indptr": np.array([0, 4, 7, 10, 13, 16]), "fn_indices": np.concatenate(faces)}


REGULAR = {
    "cart3x2": lambda: _regular("cart", (3, 2)),
    "tri2x2": lambda: _regular("tri", (2, 2)),
    "tet2x2x2": lambda: _regular("tet", (2, 2, 2)),  # the interior node has 72 records: more than a wavefront's lanes
    "tet3x3x3_perturbed": lambda: _regular("tet", (3, 3, 3), perturb=True),
    "hex2x2x2": lambda: _regular("cart", (2, 2, 2)),
    "hex3x2x2": lambda: _regular("cart", (3, 2, 2)),  # four-node faces
    "fan100": lambda: fan_2d(100),
    "fan130": lambda: fan_2d(130),  # 130 sub-faces, 260 records at the hub
}
_RAW: dict = {}


def raw_of(name: str) -> dict:
    if name not in _RAW:
        _RAW[name] = REGULAR[name]()
    return _RAW[name]


# ------------------------------------------------------------------------------------ the numpy construction
def numpy_topology(raw: dict) -> dict:
    nd = int(raw["dim"])
    cfp, cfi = np.asarray(raw["cf_indptr"], np.int64), np.asarray(raw["cf_indices"], np.int64)
    cfs = np.asarray(raw["cf_sign"], np.int8)
    fnp, fni = np.asarray(raw["fn_indptr"], np.int64), np.asarray(raw["fn_indices"], np.int64)
    nc, nf, nn = cfp.size - 1, fnp.size - 1, np.asarray(raw["nodes"]).shape[1]
    ncf, nsf = cfi.size, fni.size
    cell_of_e = np.repeat(np.arange(nc), np.diff(cfp))
    nnodes_f = np.diff(fnp)
    # (cell, face, node) triples in entry order, then stable by node
    cnt_e = nnodes_f[cfi]
    ent = np.repeat(np.arange(ncf), cnt_e)
    within = np.arange(ent.size) - np.repeat(np.cumsum(cnt_e) - cnt_e, cnt_e)
    node = fni[fnp[cfi[ent]] + within]
    order = np.lexsort((ent, node))
    ent, node = ent[order], node[order]
    nh = ent.size
    out = {"nh": nh, "node_hptr": np.searchsorted(node, np.arange(nn + 1)).astype(np.int32),
           "h_cell": cell_of_e[ent].astype(np.int32), "h_sgn": cfs[ent]}
    h_face = cfi[ent]
    # sub-faces by node
    sf_face = np.repeat(np.arange(nf), nnodes_f)
    node_sf = np.lexsort((np.arange(nsf), fni))
    fptr = np.searchsorted(fni[node_sf], np.arange(nn + 1))
    sf_ls = np.empty(nsf, np.int64)
    sf_ls[node_sf] = np.arange(nsf) - np.repeat(fptr[:-1], np.diff(fptr))
    node_face = sf_face[node_sf]
    nsides = np.bincount(cfi, minlength=nf)
    face_first = np.full(nf, np.iinfo(np.int64).max)
    np.minimum.at(face_first, cfi, cell_of_e)
    # local face index of every record: position of (node, face) among the (node, face) pairs, which are unique
    pair = node_face + nf * np.repeat(np.arange(nn), np.diff(fptr))
    assert np.array_equal(np.unique(pair), pair)
    pos = np.searchsorted(pair, h_face + nf * node)
    assert np.array_equal(pair[pos], h_face + nf * node)
    out.update(h_lf=(pos - fptr[node]).astype(np.uint8), h_first=(cell_of_e[ent] == face_first[h_face]).astype(np.uint8),
               node_fptr=fptr.astype(np.int32), node_sf=node_sf.astype(np.int32), sf_face=sf_face.astype(np.int32),
               sf_ls=sf_ls.astype(np.uint8), face_nsides=nsides.astype(np.int32), node_face=node_face.astype(np.int32))
    bnd = nsides[node_face] == 1
    n_v, cnt_v = np.diff(fptr), np.diff(out["node_hptr"]).astype(np.int64)
    nb_v = np.bincount(np.repeat(np.arange(nn), n_v)[bnd], minlength=nn)
    out["node_bptr"] = np.concatenate(([0], np.cumsum(nb_v))).astype(np.int32)
    out["node_bfaces"] = node_face[bnd].astype(np.int32)
    out["node_bls"] = sf_ls[node_sf][bnd].astype(np.uint8)
    tab = (n_v + 1) * ((cnt_v + 1) & ~1)
    out["node_tptr"] = np.concatenate(([0], np.cumsum(tab))).astype(np.int64)
    out["node_tbptr"] = np.concatenate(([0], np.cumsum(2 * n_v * nb_v))).astype(np.int64)
    out["node_cells"] = out["h_cell"][::nd][: nh // nd]
    # face order: Morton code of the face centres, stable
    fc = np.asarray(raw["face_centers"], float)
    code = np.zeros(nf, np.uint32)
    for d in range(3):
        lo, ext = fc[d].min(), fc[d].max() - fc[d].min()
        sc = 1023.999 / ext if ext > 0 else 0.0
        x = ((fc[d] - lo) * sc).astype(np.uint32) & np.uint32(0x3FF)
        x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
        x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
        x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
        x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
        code |= x << np.uint32(d)
    out["face_order"] = np.argsort(code, kind="stable").astype(np.int32)
    cls = np.minimum(np.searchsorted(CLASS_BOUNDS, n_v), CLASS_BOUNDS.size - 1)
    out["node_order"] = np.argsort(cls, kind="stable").astype(np.int32)
    out["class_begin"] = np.searchsorted(np.sort(cls), np.arange(CLASS_BOUNDS.size + 1)).astype(np.int64)
    deg = cnt_v // nd
    flops = (2.0 * n_v * n_v * n_v + 2.0 * nd * n_v * cnt_v + 2.0 * (1 + nd) * n_v * nb_v + 60.0 * nd * nd * deg).sum()
    out.update(max_face_nodes=int(nnodes_f.max()), max_cell_faces=int(np.diff(cfp).max()), max_block=int(n_v.max()),
               max_deg=int(deg.max()), max_bnd_per_node=int(nb_v.max()), sum_block_sq=int((n_v * n_v).sum()),
               tab_len=int(tab.sum()), tabb_len=int((2 * n_v * nb_v).sum()),
               node_flops_bits=int(np.float64(flops).view(np.int64)), stats_num_nodes=nn, stats_num_sub_half_faces=nh,
               stats_sum_block_sq=int((n_v * n_v).sum()), stats_max_block=int(n_v.max()),
               stats_node_table_doubles=int(tab.sum() + (2 * n_v * nb_v).sum()))
    return out


# ------------------------------------------------------------------------------------ running the library
def _params(raw: dict):
    nc = np.asarray(raw["cell_centers"]).shape[1]
    nf = np.asarray(raw["face_centers"]).shape[1]
    rng = np.random.default_rng(3)
    perm = np.zeros((3, 3, nc))
    for d in range(3):
        perm[d, d] = 1.0 + rng.random(nc)
    perm[0, 1] = perm[1, 0] = 0.1 * rng.random(nc)
    nsides = np.bincount(np.asarray(raw["cf_indices"], np.int64), minlength=nf)
    flags = np.where(nsides == 1, 1, 8).astype(np.uint8)  # Dirichlet on the boundary, internal elsewhere
    return perm, flags


def context(lib, raw: dict):
    ctx = pa.Context(0, lib)
    ctx.set_grid(raw)
    ctx.set_params(*_params(raw), None, 0.0, None)
    return ctx


# The hub of this fan is past what the SYMBOLIC phase covers (2 nodes per face x 130 cells > 254 pairs around a face): the
# topology is built and left on the handle, then the discretization stops with that message.
TOPOLOGY_ONLY = {"fan130": "more than 254 (node, cell) pairs around one face"}


def rebuilt(ctx, legacy: bool, stops_with: str | None = None) -> dict:
    with topo_path(legacy):
        if stops_with is None:
            ctx.discretize(rebuild_topology=True)
        else:
            with pytest.raises(pa.PorefvError, match=stops_with.replace("(", r"\(").replace(")", r"\)")) as e:
                ctx.discretize(rebuild_topology=True)
            assert e.value.status == 5
    return ctx.debug_topology()


def assert_same(a: dict, b: dict, what: str, keys=None):
    for k in keys or (ARRAYS + SCALARS):
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def check_case(lib, name: str):
    raw = raw_of(name)
    ref = numpy_topology(raw)
    ctx_new, ctx_old = context(lib, raw), context(lib, raw)
    stop = TOPOLOGY_ONLY.get(name)
    new, old = rebuilt(ctx_new, False, stop), rebuilt(ctx_old, True, stop)
    assert_same(new, old, f"{name}: node-cooperative vs reference path")  # (the digest is one of the scalars)
    assert new["topology_digest"] != 0
    assert new["topology_path"] == 1 and old["topology_path"] == 0  # (no silent hand-over to the reference path)
    assert ctx_new.stats()["topology_reference_path"] == 0 and ctx_old.stats()["topology_reference_path"] == 1
    if name == "fan130":  # the hub is past one pass of a wavefront's lanes
        assert new["max_block"] == 130 and new["node_hptr"][1] - new["node_hptr"][0] == 260
    keys = [k for k in ARRAYS + SCALARS if k != "topology_digest"]
    assert_same(old, ref, f"{name}: reference path vs numpy", keys)
    assert_same(new, ref, f"{name}: node-cooperative vs numpy", keys)
    ctx_new.close()
    ctx_old.close()
    return new


def check_error(lib, raw: dict, status: int, message: str):
    """The same error code and message from both paths."""
    seen = []
    for legacy in (False, True):
        ctx = context(lib, raw)
        with pytest.raises(pa.PorefvError) as e, topo_path(legacy):
            ctx.discretize(rebuild_topology=True)
        seen.append((e.value.status, e.value.message))
        ctx.close()
    assert seen[0] == seen[1], seen
    assert seen[0][0] == status and message in seen[0][1], seen


def check_rebuild_sequence(lib):
    """Rebuild twice on one handle, then after set_grid with another grid: both paths leave the same topology at every
    step, and the second grid's equals that of a fresh handle."""
    a, b = raw_of("tet2x2x2"), raw_of("hex3x2x2")
    ctxs = {legacy: context(lib, a) for legacy in (False, True)}
    for step in range(2):
        got = {legacy: rebuilt(ctx, legacy) for legacy, ctx in ctxs.items()}
        assert got[False]["topology_path"] == 1 and got[True]["topology_path"] == 0
        assert_same(got[False], got[True], f"rebuild {step}")
        assert_same(got[False], numpy_topology(a), f"rebuild {step} vs numpy",
                    [k for k in ARRAYS + SCALARS if k != "topology_digest"])
    for ctx in ctxs.values():
        ctx.set_grid(b)
        ctx.set_params(*_params(b), None, 0.0, None)
    got = {legacy: rebuilt(ctx, legacy) for legacy, ctx in ctxs.items()}
    assert_same(got[False], got[True], "after set_grid")
    assert_same(got[False], numpy_topology(b), "after set_grid vs numpy",
                [k for k in ARRAYS + SCALARS if k != "topology_digest"])
    for ctx in ctxs.values():
        ctx.close()


def check_matrices_bit_identical(lib):
    """The six MPFA matrices of the perturbed 3 x 3 x 3 tetrahedra, bit for bit between the paths."""
    raw = raw_of("tet3x3x3_perturbed")
    mats = {}
    for legacy in (False, True):
        ctx = context(lib, raw)
        with topo_path(legacy):
            ctx.discretize(rebuild_topology=True)
        mats[legacy] = [ctx.matrix(w) for w in range(6)]
        ctx.close()
    for w, (m0, m1) in enumerate(zip(mats[False], mats[True])):
        assert np.array_equal(m0.indptr, m1.indptr) and np.array_equal(m0.indices, m1.indices), w
        assert np.array_equal(m0.data, m1.data), w
