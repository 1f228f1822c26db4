"""The device CSR algebra (DeviceCsr, csrc/csr_algebra.inc) at its lane-group and class edges, shared by the
CPU suite (host-emulation library, tests/test_device_csr_edges.py) and the GPU suite (gfx950 library,
tests/test_gpu_device_csr.py).

tests/_device_csr_cases.py compares with scipy bit for bit at whatever sizes seven random draws below 120 produce.  On
the emulation build a work item is one lane: the bitonic network, the run heads found by neighbouring lanes, the keep
mask built with atomicOr, the compaction by popcount over mask words and the four rows of different length that share
one wavefront run on the device only -- and only at the row lengths of those draws.  Here every input is built
explicitly (a fixed seed gives the VALUES only, nothing is drawn with ``sps.random``) so that the row of A B that a case
is about is fed by exactly the number of products the case names, in a gather order the case knows; ``make_pair``
asserts those counts from ``indptr``.  The reference is scipy on the same canonical inputs, compared with ``same``:
pattern, indices and data bit for bit.  Every product case asserts ``stats()["spgemm_path"]`` (16 / 32 / 64: sorted
in LDS with that many lanes per row; 1: the global radix sorts) and the LDS bytes of its launch, so that it cannot
silently run another class; the emulation build computes both the way the device does.

Values are +-(1 + u) 2^k with k in -20 ... 20: the order of accumulation inside a run of equal columns changes the bits
of its sum.  ``assert_discriminates`` checks that on the host (the forward sum of at least one run of three or more
products differs from the sum in reversed order) in every case that has such runs: inputs for which it failed would
not tell gather order from any other.

``CASES`` is the list both suites run; ``EMULATION_ONLY`` are the malformed ``indptr`` inputs (see
``abi_indptr_is_checked_on_the_host``)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import porepy_amd as pa
from porepy_amd import _lib
from porepy_amd import device_csr as dc
from tests._device_csr_cases import flow_problem, same

MAX_LDS_ROW = 4096   # kSpgemmMaxRow of csr_algebra.inc
OPT_IN = 48 * 1024   # dynamic LDS beyond which a launch has to opt in (hipFuncSetAttribute, backend.h: wave_for)


# ------------------------------------------------------------------------------------------------------ the inputs
def values(rng, n):
    """+-(1 + u) 2^k, k in -20 ... 20"""
    return rng.choice([-1.0, 1.0], n) * (1.0 + rng.random(n)) * np.exp2(rng.integers(-20, 21, n))


def make_pair(rows, ncols, seed=0):
    """A and B (canonical csr, int32 indices) such that row r of A B is fed by ``len(rows[r])`` products whose columns, in
    gather order (scipy's csr_matmat: k in the storage order of row r of A, j in that of row k of B), are ``rows[r]``.
    An item of a row is a column or ``(column, value)``.  The plan of a row is cut into its maximal strictly increasing
    segments; every segment becomes one row of B, and row r of A holds one entry per segment.  The factor in A is 1.0 for
    a segment with an explicit value (the product then IS that value) and drawn otherwise, as are the values in B."""
    rng = np.random.default_rng(seed)
    a_ptr, a_idx, a_val, b_ptr, b_idx, b_val = [0], [], [], [0], [], []
    for plan in rows:
        seg = []

        def flush():
            if not seg:
                return
            drawn = values(rng, len(seg) + 1)
            a_idx.append(len(b_ptr) - 1)
            a_val.append(1.0 if any(v is not None for _, v in seg) else drawn[-1])
            for (c, v), d in zip(seg, drawn):
                b_idx.append(c)
                b_val.append(d if v is None else v)
            b_ptr.append(len(b_idx))
            seg.clear()

        for item in plan:
            c, v = item if isinstance(item, tuple) else (item, None)
            if seg and c <= seg[-1][0]:
                flush()
            seg.append((int(c), v))
        flush()
        a_ptr.append(len(a_idx))
    nb = max(len(b_ptr) - 1, 1)
    b_ptr = b_ptr if len(b_ptr) > 1 else [0, 0]
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    A = sps.csr_matrix((np.asarray(a_val, dtype=np.float64), i32(a_idx), i32(a_ptr)), shape=(len(rows), nb))
    B = sps.csr_matrix((np.asarray(b_val, dtype=np.float64), i32(b_idx), i32(b_ptr)), shape=(nb, ncols))
    for M in (A, B):
        assert is_canonical(M)
    assert list(products_per_row(A, B)) == [len(p) for p in rows]
    return A, B


def is_canonical(M):
    """rows sorted by column without duplicates, indices in range: read off the arrays, not scipy's cached flag"""
    ip, ix = M.indptr, M.indices.astype(np.int64)
    if ip[0] != 0 or ip[-1] != ix.size or np.any(np.diff(ip) < 0) or np.any(ix < 0) or np.any(ix >= M.shape[1]):
        return False
    inner = np.ones(ix.size, dtype=bool)
    inner[ip[:-1][np.diff(ip) > 0]] = False  # (the first entry of a row has no left neighbour)
    return bool(np.all(np.diff(ix)[inner[1:]] > 0))


def products_per_row(A, B):
    """the number of products feeding every row of A B, from the index arrays alone"""
    ones = sps.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    return np.rint(ones @ np.diff(B.indptr).astype(np.float64)).astype(np.int64)


def gathered(A, B, r):
    """columns and values of the products of row r in gather order"""
    cols, vals = [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
    for e in range(A.indptr[r], A.indptr[r + 1]):
        sl = slice(B.indptr[A.indices[e]], B.indptr[A.indices[e] + 1])
        cols.append(B.indices[sl].astype(np.int64))
        vals.append(A.data[e] * B.data[sl])
    return np.concatenate(cols), np.concatenate(vals)


def sorted_runs(A, B, r):
    """[(sorted position of the head, column, products in gather order)] of row r, as the sort by (column, gather
    position) lays the runs out"""
    cols, vals = gathered(A, B, r)
    order = np.argsort(cols, kind="stable")
    cols, vals = cols[order], vals[order]
    heads = np.flatnonzero(np.r_[True, cols[1:] != cols[:-1]]) if cols.size else np.zeros(0, dtype=np.int64)
    ends = np.r_[heads[1:], cols.size]
    return [(int(h), int(cols[h]), vals[h:e]) for h, e in zip(heads, ends)]


def forward_sum(v):
    return np.cumsum(v)[-1]  # (cumsum adds one after the other, as the kernels and scipy do)


def dropped_heads(A, B, r):
    return [h for h, _, v in sorted_runs(A, B, r) if forward_sum(v) == 0.0]


def discriminates(A, B):
    """the inputs tell gather order from another order: there are runs of three or more products, and the forward sum of
    at least one of them differs from its sum in reversed order"""
    long_runs = [v for r in range(A.shape[0]) for _, _, v in sorted_runs(A, B, r) if v.size >= 3]
    assert long_runs, "no run of three or more products"
    return any(forward_sum(v) != forward_sum(v[::-1]) for v in long_runs)


def assert_discriminates(A, B):
    assert discriminates(A, B), "the inputs do not discriminate"


def discriminating_pair(rows, ncols, seed):
    """make_pair with the values of the first seed from ``seed`` on that discriminate (a sum of few terms of very
    different size is often the same in both orders)"""
    for s in range(seed, seed + 32):
        A, B = make_pair(rows, ncols, s)
        if discriminates(A, B):
            return A, B
    raise AssertionError("no seed whose values discriminate")


def hashed_plan(m, width=None):
    """m products spread over ``width`` columns (default m // 3 + 1: runs of about three) in a fixed scrambled order:
    segments of every short length"""
    width = m // 3 + 1 if width is None else width
    return [int((t * 2654435761) % 4294967296 % width) for t in range(m)]


def ramp_plan(m, width=24):
    """columns 0 ... width - 1 over and over: few, long segments (a B of a few rows)"""
    return [t % width for t in range(m)]


def scrambled(runs, prime=1009):
    """the plan of a row from its runs [(column, [value or None, ...])]: the products ordered by a fixed permutation of the
    columns, those of one run next to each other in the order given (equal columns: one segment each)"""
    assert all(c < prime for c, _ in runs)
    items = [(c, v) for c, vs in runs for v in vs]
    return sorted(items, key=lambda it: (it[0] * 73) % prime)  # (stable: the order inside a run is kept)


# -------------------------------------------------------------------------------------------- what a product must be
def lds_bytes(m, lanes):
    """dynamic LDS of the workgroup that sorts rows of up to m products with ``lanes`` lanes each (csr_spgemm: keys,
    values, mask words and 64 spare bytes per row; wave_for rounds a row's share up to 16 bytes and puts 64 / lanes rows
    into one single-wavefront workgroup)"""
    cap_l = max(m, 1)
    cap_p = 2
    while cap_p < cap_l:
        cap_p *= 2
    per_row = 8 * cap_p + 8 * cap_l + 8 * (cap_p // 64 + 1) + 64
    return (per_row + 15) // 16 * 16 * (64 // lanes)


def expected_path(m):
    return 16 if m <= 64 else 32 if m <= 160 else 64 if m <= MAX_LDS_ROW else 1


def product(ctx, A, B):
    C = (pa.DeviceCsr.from_scipy(A, ctx) @ pa.DeviceCsr.from_scipy(B, ctx)).to_scipy()
    st = ctx.stats()
    return C, int(st["spgemm_path"]), int(st["spgemm_lds_bytes"])


def check_product(ctx, A, B, generic=None, monkeypatch=None):
    """A B on the path its longest row selects: the bits of scipy's product, the path and the LDS bytes of that class.
    ``generic`` (with monkeypatch): the same through the global sorts too -- same bits again."""
    longest = int(products_per_row(A, B).max()) if A.shape[0] else 0
    ref = A @ B
    C, path, lds = product(ctx, A, B)
    print(f"{A.shape[0]} rows, longest fed by {longest} products: spgemm_path {path}, spgemm_lds_bytes {lds}")
    assert path == expected_path(longest)
    assert lds == (lds_bytes(longest, path) if path != 1 else 0)
    same(C, ref)
    if generic:
        monkeypatch.setenv("PFV_SPGEMM_GENERIC", "1")
        try:
            Cg, path_g, lds_g = product(ctx, A, B)
        finally:
            monkeypatch.delenv("PFV_SPGEMM_GENERIC")
        assert (path_g, lds_g) == (1, 0)
        same(Cg, ref)
        same(Cg, C)
    return C


class Hooks:
    """vectors on the device: ``to_device(array) -> (address, keepalive)``, ``from_device(keepalive) -> array``; the
    emulation build works on host addresses (as ``_parity.device_resident_vectors``)"""

    def __init__(self, to_device=None, from_device=None):
        self.to_device = to_device or (lambda a: (a.ctypes.data, a))
        self.from_device = from_device or (lambda keep: keep)


# ------------------------------------------------------------------------------------------ product, LDS path: edges
EDGE_COUNTS = [1, 2, 3, 16, 17, 63, 64, 65, 128, 129, 160, 161, 255, 256, 257, 1023, 1024, 1025, 1975, 1976, 2048, 2049,
               4095, 4096]


def edge_pair(m, seed=1):
    rows = [hashed_plan(min(m, 3)), hashed_plan(m), [], hashed_plan(m // 2)]
    return make_pair(rows, m // 3 + 3, seed)


def product_class_edge(lib, monkeypatch, hooks, m):
    """The longest row is fed by m products: 16 lanes up to 64, 32 up to 160, 64 beyond; capP doubles at every power of
    two, a mask word starts every 64 products.

    The opt-in to more than 48 KiB of LDS.  With 64 lanes a workgroup sorts one row and needs
    8 capP + 8 m + 8 (capP / 64 + 1) + 64 bytes, rounded up to 16:
        m = 1975, 1976 (capP = 2048):  32 512 and 32 528 bytes -- both below 49 152;
        m = 2048       (capP = 2048):  33 104 bytes, the most a row of the 2048 class needs;
        m = 2049       (capP = 4096):  49 744 bytes, the first launch that opts in.
    The edge lies at 2048 | 2049 because capP doubles there.  (1975 | 1976 is where 8 * 4096 + 8 m + 8 * 65 + 64 crosses
    49 152, but no row of fewer than 2049 products has capP = 4096: 1976 stays below the limit, and is asserted to.)"""
    ctx = pa.Context(0, lib)
    A, B = edge_pair(m)
    if m >= 16:
        assert_discriminates(A, B)
    check_product(ctx, A, B)
    lds = int(ctx.stats()["spgemm_lds_bytes"])
    assert (lds_bytes(1975, 64), lds_bytes(1976, 64), lds_bytes(2048, 64), lds_bytes(2049, 64)) == (32512, 32528, 33104, 49744)
    if m <= 2048:
        assert lds <= OPT_IN
    else:
        assert lds > OPT_IN
    ctx.close()


def product_4096_forced_and_4097(lib, monkeypatch, hooks):
    """4096 | 4097: the last row sorted in LDS and the first that takes the global sorts; the 4096 matrix forced through
    the global sorts (PFV_SPGEMM_GENERIC=1) gives the bits of the LDS path"""
    ctx = pa.Context(0, lib)
    A, B = edge_pair(4096)
    check_product(ctx, A, B, generic=True, monkeypatch=monkeypatch)
    A, B = edge_pair(4097)
    assert_discriminates(A, B)
    C, path, lds = product(ctx, A, B)
    assert (path, lds) == (1, 0)
    same(C, A @ B)
    ctx.close()


# ------------------------------------------------------------------------- product, LDS path: rows sharing a wavefront
def p2_of(m):
    p = 2
    while p < m:
        p *= 2
    return p


def mixed_lengths(lanes, limit=None):
    """an empty row, rows of 1 and 2 products, every power of two and power of two plus one up to the class limit, the
    limit itself first (it selects the class whatever prefix of the rows is taken), ordered so that the rows that share a
    wavefront (64 / lanes neighbours) differ in the size P2 of their sorting network"""
    limit = {16: 64, 32: 160, 64: MAX_LDS_ROW}[lanes] if limit is None else limit
    lens = {0, 1, 2, limit}
    p = 2
    while p <= limit:
        lens |= {p} | ({p + 1} if p + 1 <= limit else set())
        p *= 2
    rest = sorted(lens - {limit})
    per_block = 64 // lanes
    out = [limit]
    while rest:
        group = out[len(out) // per_block * per_block:] if len(out) % per_block else []
        pick = next((x for x in rest if p2_of(x) not in {p2_of(g) for g in group}), rest[0])
        rest.remove(pick)
        out.append(pick)
    for i in range(0, len(out) - per_block + 1, per_block):
        assert len({p2_of(x) for x in out[i:i + per_block]}) == per_block, (lanes, out)
    return out


def product_mixed_rows(lib, monkeypatch, hooks, lanes, n):
    """rows of different length in one wavefront (four at 16 lanes, two at 32): different trip counts of the network
    around w.sync(); n = 1, 3, 4, 5 rows (a partly filled wavefront) and all of them"""
    ctx = pa.Context(0, lib)
    lens = mixed_lengths(lanes)
    lens = lens if n == "all" else lens[:n]
    A, B = make_pair([hashed_plan(m) for m in lens], max(lens) // 3 + 3, seed=lanes)
    assert_discriminates(A, B)
    check_product(ctx, A, B)
    assert int(ctx.stats()["spgemm_path"]) == lanes
    ctx.close()


def product_second_grid_trip(lib, monkeypatch, hooks, lanes):
    """n = 256 * 64 * (64 / lanes) + 3 rows: the launch has 16 384 workgroups (backend.h: wave_for), so the grid-stride
    loop runs a second trip whose last workgroup is partly empty.  One row pattern repeated (for 64 lanes: up to 300
    products, just inside the class), plans of long segments so that B has a few dozen rows."""
    ctx = pa.Context(0, lib)
    n = 256 * 64 * (64 // lanes) + 3
    lens = mixed_lengths(lanes, 300 if lanes == 64 else None)
    A, B = make_pair([ramp_plan(m) for m in lens], 24, seed=lanes + 1)
    assert_discriminates(A, B)
    reps = -(-n // len(lens))
    big = sps.vstack([A] * reps, format="csr")[:n]
    big = sps.csr_matrix((big.data, big.indices.astype(np.int32), big.indptr.astype(np.int32)), shape=big.shape)
    assert big.shape[0] == n and is_canonical(big)
    check_product(ctx, big, B)
    assert int(ctx.stats()["spgemm_path"]) == lanes
    ctx.close()


# ------------------------------------------------------------------------------------ product: runs and the keep mask
def single_run_pair(m):
    """all m products of the middle row land on column 5: one run, summed in gather order"""
    rows = [[1, 2], [5] * m, [0, 5, 6]]
    return discriminating_pair(rows, 8, seed=m) if m >= 3 else make_pair(rows, 8, seed=m)


def cancel_pair(m=200):
    """Rows of m sorted positions, all single products but one run that is dropped: a pair that cancels exactly with its
    head at sorted position 0, 63, 64, 65, 127, 128 and m - 2 (the last place a run of two can start), and -- the head
    at m - 1 itself -- a single product whose value is an exact zero (a stored zero in B; scipy drops the entry too)."""
    rows, where = [], [0, 63, 64, 65, 127, 128, m - 2, m - 1]
    v = 1.390625 * 2.0 ** -7
    for p in where:
        runs = [(c, [None]) for c in range(p)]
        runs += [(p, [0.0])] if p == m - 1 else [(p, [v, -v])]
        runs += [(c, [None]) for c in range(p + 1, m - (1 if p < m - 1 else 0))]
        rows.append(scrambled(runs))
    A, B = make_pair(rows, m + 1, seed=11)
    assert list(products_per_row(A, B)) == [m] * len(where)
    assert [dropped_heads(A, B, r) for r in range(len(where))] == [[p] for p in where]
    return A, B


def alternating_pair(m=200):
    """m sorted positions, keep / drop alternating: in row 0 every odd position is a single exact zero, in row 1 every
    kept single is followed by a pair that cancels -- kept heads in the mask words 0 ... 3, so that the position of a
    kept entry needs the prefix over the earlier words"""
    v = 1.171875 * 2.0 ** 3
    row0 = [(c, [None] if c % 2 == 0 else [0.0]) for c in range(m)]
    row1 = []
    for c in range(0, 2 * (m // 3), 2):
        row1 += [(c, [None]), (c + 1, [v, -v])]
    row1 += [(2 * (m // 3) + i, [None]) for i in range(m - 3 * (m // 3))]
    A, B = make_pair([scrambled(row0), scrambled(row1)], m + 1, seed=12)
    assert list(products_per_row(A, B)) == [m, m]
    assert dropped_heads(A, B, 0) == list(range(1, m, 2))
    assert dropped_heads(A, B, 1) == list(range(1, 3 * (m // 3), 3))
    return A, B


def all_cancel_pair():
    """every run of the middle row cancels: an empty result row between two non-empty ones"""
    v = 1.65625 * 2.0 ** 9
    runs = [(c, [v * (c + 1), -v * (c + 1)]) for c in range(0, 40, 2)] + [(c, [0.0]) for c in range(1, 40, 2)]
    A, B = make_pair([hashed_plan(5, 40), scrambled(runs), hashed_plan(7, 40)], 41, seed=13)
    assert len(dropped_heads(A, B, 1)) == 40 and not dropped_heads(A, B, 0) and not dropped_heads(A, B, 2)
    ref = A @ B
    assert ref.indptr[1] == ref.indptr[2] and ref.indptr[1] > 0 and ref.indptr[3] > ref.indptr[2]
    return A, B


def growing_runs_pair():
    """runs of length 1, 2, 3, ..., 20 in column order"""
    A, B = make_pair([scrambled([(c, [None] * (c + 1)) for c in range(20)])], 21, seed=14)
    assert [v.size for _, _, v in sorted_runs(A, B, 0)] == list(range(1, 21))
    return A, B


KEEP_MASK_PAIRS = {"run_2": lambda: single_run_pair(2), "run_64": lambda: single_run_pair(64),
                   "run_65": lambda: single_run_pair(65), "run_130": lambda: single_run_pair(130),
                   "cancelling_pairs": cancel_pair, "alternating": alternating_pair, "all_cancel": all_cancel_pair,
                   "growing_runs": growing_runs_pair}


def product_keep_mask(lib, monkeypatch, hooks, name):
    """runs and the keep mask, through the sort in LDS and through the global sorts: scipy's bits both times"""
    ctx = pa.Context(0, lib)
    A, B = KEEP_MASK_PAIRS[name]()
    if name in ("run_64", "run_65", "run_130", "growing_runs"):
        assert_discriminates(A, B)
    check_product(ctx, A, B, generic=True, monkeypatch=monkeypatch)
    ctx.close()


# ------------------------------------------------------------------------------------------------------- product: keys
def product_keys(lib, monkeypatch, hooks):
    """the sort key: the column in the upper half (B with 2^20 + 3 columns, entries in columns 0, 2^20 and 2^20 + 2), the
    gather position in the lower half up to m - 1 = 4095"""
    ctx = pa.Context(0, lib)
    cols = [0, 2 ** 20, 2 ** 20 + 2]
    A, B = make_pair([[cols[t % 3] for t in range(4096)], [cols[2], cols[0]], [cols[1]]], 2 ** 20 + 3, seed=21)
    assert_discriminates(A, B)
    C = check_product(ctx, A, B)
    assert list(C[0].indices) == cols and int(ctx.stats()["spgemm_path"]) == 64
    ctx.close()


# ------------------------------------------------------------------------------------------ product, global-sort path
def product_generic_empty(lib, monkeypatch, hooks):
    """empty operands through the global sorts: 5 x 7 empty times 7 x 3, and 0 x 7 times 7 x 3"""
    ctx = pa.Context(0, lib)
    B = explicit_matrix(7, 3, 31, lambda i, j: (i + j) % 2 == 0)
    monkeypatch.setenv("PFV_SPGEMM_GENERIC", "1")
    for nr in (5, 0):
        Z = sps.csr_matrix((nr, 7))
        C, path, lds = product(ctx, Z, B)
        assert (path, lds) == (1, 0)
        same(C, sps.csr_matrix((nr, 3)))
        assert C.nnz == 0 and np.array_equal(C.indptr, np.zeros(nr + 1))
    monkeypatch.delenv("PFV_SPGEMM_GENERIC")
    for nr in (5, 0):  # (and the default path on the same operands)
        C, path, _ = product(ctx, sps.csr_matrix((nr, 7)), B)
        assert path == 16
        same(C, sps.csr_matrix((nr, 3)))
    ctx.close()


def product_generic_key_bits(lib, monkeypatch, hooks, ncols, n):
    """the widths cbits / rbits of the two radix sorts: B with 1, 2, 3, 2^16 and 2^16 + 1 columns (first, middle and last
    column used), 1, 2 and 3 rows of A"""
    ctx = pa.Context(0, lib)
    cols = sorted({0, ncols // 2, ncols - 1})
    plans = [[cols[t % len(cols)] for t in range(30)], list(reversed(cols)) * 8, cols * 5]
    A, B = discriminating_pair(plans[:n], ncols, seed=ncols % 97 + n)
    monkeypatch.setenv("PFV_SPGEMM_GENERIC", "1")
    C, path, lds = product(ctx, A, B)
    monkeypatch.delenv("PFV_SPGEMM_GENERIC")
    assert (path, lds) == (1, 0)
    same(C, A @ B)
    ctx.close()


# ----------------------------------------------------------------------------------------------------------- matrices
def explicit_matrix(nr, nc, seed, keep=lambda i, j: (7 * i + 3 * j) % 5 < 2):
    """nr x nc, entry (i, j) stored where ``keep`` says so; canonical, int32 indices"""
    rng = np.random.default_rng(seed)
    ij = [(i, j) for i in range(nr) for j in range(nc) if keep(i, j)]
    M = sps.csr_matrix((values(rng, len(ij)), ([i for i, _ in ij], [j for _, j in ij])), shape=(nr, nc)) if ij \
        else sps.csr_matrix((nr, nc))
    M.sort_indices()
    return sps.csr_matrix((M.data, M.indices.astype(np.int32), M.indptr.astype(np.int32)), shape=(nr, nc))


# ---------------------------------------------------------------------------------------------------------- transpose
def transpose_widths(lib, monkeypatch, hooks, ncols):
    """the key width of the sort by column (1, 2, 3, 64, 65, 2^16, 2^16 + 1 columns); an empty first and last column
    (from three columns on), a column hit by every row"""
    ctx = pa.Context(0, lib)
    hit = ncols // 2
    edge = (lambda j: 0 < j < ncols - 1) if ncols >= 3 else (lambda j: True)
    used = sorted({hit, 1, ncols - 2, ncols // 3, 2 * ncols // 3} & set(range(ncols)))
    rng = np.random.default_rng(ncols)
    rows = [[j for j in used if edge(j) and (j == hit or (i + j) % 3)] for i in range(9)]
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    A = sps.csr_matrix((values(rng, int(ptr[-1])), np.asarray(sum(rows, []), dtype=np.int32), ptr), shape=(9, ncols))
    assert is_canonical(A) and np.all(np.diff(A.tocsc().indptr)[hit] == 9)
    if ncols >= 3:
        assert A.tocsc().indptr[1] == 0 and A.tocsc().indptr[-1] == A.tocsc().indptr[-2]
    dA = pa.DeviceCsr.from_scipy(A, ctx)
    T = dA.T
    same(T.to_scipy(), A.T.tocsr())
    same(T.T.to_scipy(), A)
    ctx.close()


def transpose_empty(lib, monkeypatch, hooks):
    """a 0 x 5 and a 5 x 0 operand"""
    ctx = pa.Context(0, lib)
    for shape in ((0, 5), (5, 0)):
        Z = sps.csr_matrix(shape)
        T = pa.DeviceCsr.from_scipy(Z, ctx).T
        assert T.shape == shape[::-1] and T.nnz == 0
        same(T.to_scipy(), Z.T.tocsr())
        same(T.T.to_scipy(), Z)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- sum
def sum_cases(lib, monkeypatch, hooks):
    """A + (-1) A: nothing is left; rows where only A, only B or neither has entries; alpha or beta equal to 0 (scipy drops
    the zeros that makes: what 0.0 * A + 1.0 * B gives there)"""
    ctx = pa.Context(0, lib)
    A = explicit_matrix(12, 9, 41, lambda i, j: i % 4 in (0, 1) and (i + 2 * j) % 3 == 0)   # rows 2, 3 mod 4 empty
    B = explicit_matrix(12, 9, 42, lambda i, j: i % 4 in (0, 2) and (i + j) % 2 == 0)       # rows 1, 3 mod 4 empty
    la, lb = np.diff(A.indptr), np.diff(B.indptr)
    assert ((la > 0) & (lb > 0)).any() and ((la > 0) & (lb == 0)).any() and ((la == 0) & (lb > 0)).any() and ((la == 0) & (lb == 0)).any()
    dA, dB = pa.DeviceCsr.from_scipy(A, ctx), pa.DeviceCsr.from_scipy(B, ctx)
    Z = dA.axpby(1.0, dA, -1.0).to_scipy()
    assert Z.nnz == 0 and np.array_equal(Z.indptr, np.zeros(13))
    same(Z, A + (-1.0) * A)
    same((dA + dB).to_scipy(), A + B)
    same((dA - dB).to_scipy(), A - B)
    same(dA.axpby(0.3, dB, -1.7).to_scipy(), 0.3 * A + (-1.7) * B)
    for alpha, beta in ((0.0, 1.0), (1.0, 0.0), (0.0, 0.0), (-2.5, 0.0)):
        ref = alpha * A + beta * B  # (scipy's scalar product keeps the zeros it makes, its sum then drops every exact zero)
        C = dA.axpby(alpha, dB, beta).to_scipy()
        same(C, ref)
        dense = alpha * A.toarray() + beta * B.toarray()
        assert np.array_equal(C.toarray(), dense) and C.nnz == np.count_nonzero(dense)
    ctx.close()


# ------------------------------------------------------------------------------------------ bmat / block_diag / vstack
def block_cases(lib, monkeypatch, hooks):
    """a block row of three blocks whose rows hold 0, 1, 17 and 40 entries (more entries than the 16 lanes of the copy, the
    running offset inside a row used twice); a zero-row and a zero-column block; vstack of three matrices"""
    ctx = pa.Context(0, lib)
    counts = [0, 1, 17, 40]

    def block(seed, shift):
        return explicit_matrix(4, 45, seed, lambda i, j: j < counts[(i + shift) % 4])

    X, Y, Z = block(51, 0), block(52, 1), block(53, 2)
    assert sorted(np.diff(X.indptr)) == counts and list(np.diff(Y.indptr)) != list(np.diff(X.indptr))
    dX, dY, dZ = (pa.DeviceCsr.from_scipy(M, ctx) for M in (X, Y, Z))
    same(pa.bmat([[dX, dY, dZ]]).to_scipy(), sps.bmat([[X, Y, Z]], format="csr"))
    same(pa.bmat([[dX, None, dZ], [dY, dZ, None], [None, dX, dY]]).to_scipy(),
         sps.bmat([[X, None, Z], [Y, Z, None], [None, X, Y]], format="csr"))
    same(pa.block_diag([dX, dY, dZ]).to_scipy(), sps.block_diag([X, Y, Z], format="csr"))
    R0, C0 = sps.csr_matrix((0, 45)), sps.csr_matrix((4, 0))
    d0r, d0c = pa.DeviceCsr.from_scipy(R0, ctx), pa.DeviceCsr.from_scipy(C0, ctx)
    same(pa.bmat([[dX, d0c, dY], [d0r, None, d0r], [dZ, d0c, dX]]).to_scipy(),
         sps.bmat([[X, C0, Y], [R0, None, R0], [Z, C0, X]], format="csr"))
    same(pa.block_diag([dX, d0r, d0c, dY]).to_scipy(), sps.block_diag([X, R0, C0, Y], format="csr"))
    same(pa.vstack([dX, dY, dZ]).to_scipy(), sps.vstack([X, Y, Z], format="csr"))
    same(pa.vstack([dX, d0r, dZ]).to_scipy(), sps.vstack([X, R0, Z], format="csr"))
    same(pa.vstack([X, dY, Z]).to_scipy(), sps.vstack([X, Y, Z], format="csr"))  # (host operands are uploaded)
    ctx.close()


# ------------------------------------------------------------------------------------ operators the reference's AdArray calls
def operator_row_selection(lib, monkeypatch, hooks):
    """J[slice], J[index array with repeats], J[bool mask], J[int] against scipy's row selection; J[:, 1] is refused"""
    ctx = pa.Context(0, lib)
    M = explicit_matrix(37, 29, 61)
    J = pa.DeviceCsr.from_scipy(M, ctx)
    mask = np.arange(37) % 3 == 1
    for key in (slice(3, 30, 2), slice(None, None, -1), slice(5, 5), np.array([5, 5, 0, 36, 5, 17]), mask):
        S = J[key]
        same(S.to_scipy(), M[key])
    S = J[7]
    assert S.shape == (1, 29)
    same(S.to_scipy(), M[[7]])
    same(J[-1].to_scipy(), M[[36]])
    with pytest.raises(IndexError):
        J[:, 1]
    ctx.close()


def operator_division(lib, monkeypatch, hooks):
    """J / s as scipy computes it (the product with the rounded reciprocal), for s = 3.0 and s = 1e-300; for s = 3.0 that
    is NOT the true division, in at least one entry"""
    ctx = pa.Context(0, lib)
    M = explicit_matrix(37, 29, 62)
    J = pa.DeviceCsr.from_scipy(M, ctx)
    assert np.array_equal((M / 3.0).data, M.data * (1.0 / 3.0)) and not np.array_equal((M / 3.0).data, M.data / 3.0)
    for s in (3.0, 1e-300):
        same((J / s).to_scipy(), M / s)
    same(J.to_scipy(), M)  # (a new matrix: the operand is unchanged)
    assert J.__truediv__(np.ones(3)) is NotImplemented
    ctx.close()


def operator_scipy_operands(lib, monkeypatch, hooks):
    """scipy on the left: sps.diags(v) * J and J * sps.diags(v) (row / column scaling), M @ J for a csr M and for
    M = sps.diags(v), M + J, M - J; J.copy() is a matrix of its own"""
    ctx = pa.Context(0, lib)
    rng = np.random.default_rng(63)
    M = explicit_matrix(37, 29, 63)
    J = pa.DeviceCsr.from_scipy(M, ctx)
    vr, vc = values(rng, 37), values(rng, 29)
    for res, ref in ((sps.diags(vr) * J, sps.diags(vr) @ M), (J * sps.diags(vc), M @ sps.diags(vc)),
                     (sps.diags(vr) @ J, sps.diags(vr) @ M)):
        assert isinstance(res, pa.DeviceCsr)
        same(res.to_scipy(), ref)
    L = explicit_matrix(11, 37, 64, lambda i, j: (i + j) % 4 == 0)
    res = L @ J
    assert isinstance(res, pa.DeviceCsr)
    same(res.to_scipy(), L @ M)
    assert_discriminates(L, M)
    K = explicit_matrix(37, 29, 65, lambda i, j: (5 * i + j) % 3 == 0)
    for res, ref in ((K + J, K + M), (K - J, K - M), (J + K, M + K), (J - K, M - K)):
        assert isinstance(res, pa.DeviceCsr)
        same(res.to_scipy(), ref)
    cp = J.copy()
    assert cp is not J and cp._c.value != J._c.value and cp.shape == J.shape and cp.nnz == J.nnz
    same(cp.to_scipy(), M)
    ctx._check(ctx.lib.pfv_csr_scale(cp._c, _lib._ptr(vr, _lib._dp), None))  # in place, on the copy
    same(cp.to_scipy(), sps.diags(vr) @ M)
    same(J.to_scipy(), M)
    ctx.close()


def tridiagonal(n, seed):
    rng = np.random.default_rng(seed)
    return sps.diags([-1.0 - 0.5 * rng.random(n - 1), 4.0 + rng.random(n), -1.0 - 0.5 * rng.random(n - 1)], [-1, 0, 1],
                     format="csr")


def operator_device_vectors(lib, monkeypatch, hooks):
    """matvec_device on device vectors: y against the longdouble product within (len_i + 2) 2^-53 (|A| |x|)_i per row (one
    rounding per product, len_i - 1 per sum in any order, one to spare); as_system(rhs_device_ptr=...): the system and
    the solution of the host-array call"""
    ctx = pa.Context(0, lib)
    rng = np.random.default_rng(66)
    M = explicit_matrix(70, 53, 66, lambda i, j: j < [0, 1, 17, 40, 53][i % 5] and (i + j) % 2 == 0 or j == i % 53 and i % 5 > 0)
    J = pa.DeviceCsr.from_scipy(M, ctx)
    x = values(rng, 53)
    px, kx = hooks.to_device(np.ascontiguousarray(x))
    py, ky = hooks.to_device(np.full(70, np.nan))
    J.matvec_device(px, py)
    ctx.sync()
    y = np.asarray(hooks.from_device(ky))
    exact = np.array([np.sum(M.data[M.indptr[i]:M.indptr[i + 1]].astype(np.longdouble)
                             * x[M.indices[M.indptr[i]:M.indptr[i + 1]]].astype(np.longdouble)) for i in range(70)])
    bound = (np.diff(M.indptr) + 2) * 2.0 ** -53 * (abs(M) @ abs(x))
    err = np.abs(y.astype(np.longdouble) - exact).astype(np.float64)
    print(f"matvec_device: worst error / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}")
    assert np.all(err <= bound) and np.all(y[np.diff(M.indptr) == 0] == 0.0)
    assert np.array_equal(J @ x, y)  # (the host-vector product is the same kernel)

    T = tridiagonal(50, 67)
    b = values(rng, 50)
    dT = pa.DeviceCsr.from_scipy(T, ctx)
    host = pa.Context(0, lib)
    xh, ih = dT.as_system(b, context=host).solve("bicgstab", rtol=1e-12, n=50, precond="jacobi")
    dev = pa.Context(0, lib)
    pb, kb = hooks.to_device(np.ascontiguousarray(b))
    s = dT.as_system(None, context=dev, rhs_device_ptr=pb)
    assert s is dev and np.array_equal(dev.rhs(), b)
    xd, idv = dev.solve("bicgstab", rtol=1e-12, n=50, precond="jacobi")
    assert idv["iterations"] == ih["iterations"] and np.array_equal(xd, xh)
    x_ref = spla.spsolve(T.tocsc(), b)
    assert np.linalg.norm(xd - x_ref) <= 1e-9 * np.linalg.norm(x_ref)
    for c in (host, dev, ctx):
        c.close()


# ------------------------------------------------------------------------------------------------ routes to the solver
def routes_to_the_solver(lib, monkeypatch, hooks):
    """J = div @ flux of flow_problem(4) built by the product in LDS, by the forced global sorts and by
    from_scipy(J.to_scipy()): the three carry different max_row (the LDS path records the bound maxcap, the others the
    longest row).  Each solved through as_system with BiCGStab under AMG and under Jacobi, on a fresh handle: the same
    iteration count and the same bits of x for the three routes -- nothing may size or select itself by max_row -- and
    x within 1e-9 of scipy's direct solve."""
    g, data = flow_problem(4)
    d = pa.Mpfa("flow", library=lib, lazy=True)
    d.discretize(g, data)
    mats = data[pa.DISCRETIZATION_MATRICES]["flow"]
    ctx = d.context(g)
    flux = pa.DeviceCsr.from_any(mats["flux"], ctx)
    bound_flux = pa.DeviceCsr.from_any(mats["bound_flux"], ctx)
    div = pa.DeviceCsr.from_scipy(sps.csr_matrix(g.cell_faces.T), ctx)
    J_lds = div @ flux
    assert int(ctx.stats()["spgemm_path"]) in (16, 32, 64)
    monkeypatch.setenv("PFV_SPGEMM_GENERIC", "1")
    J_glob = div @ flux
    monkeypatch.delenv("PFV_SPGEMM_GENERIC")
    assert int(ctx.stats()["spgemm_path"]) == 1
    Jh = J_lds.to_scipy()
    same(J_glob.to_scipy(), Jh)
    J_host = pa.DeviceCsr.from_scipy(Jh, ctx)
    rhs = -(div @ (bound_flux @ data[pa.PARAMETERS]["flow"]["bc_values"]))
    x_ref = spla.spsolve(Jh.tocsc(), rhs)
    for precond in ("amg", "jacobi"):
        got = []
        for J in (J_lds, J_glob, J_host):
            solver = pa.Context(0, lib)
            x, info = J.as_system(rhs, context=solver).solve("bicgstab", rtol=1e-12, maxit=2000, n=g.num_cells, precond=precond)
            got.append((x, info["iterations"]))
            solver.close()
        print(f"{precond}: iterations {[it for _, it in got]}")
        assert got[0][1] == got[1][1] == got[2][1]
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][0], got[2][0])
        assert np.linalg.norm(got[0][0] - x_ref) <= 1e-9 * np.linalg.norm(x_ref)


# ------------------------------------------------------------------------------------------------------- upload cache
def upload_cache(lib, monkeypatch, hooks):
    """from_any remembers the upload of a host matrix while its arrays -- values, indices AND indptr -- are what they were:
    a permutation matrix (unit values) whose columns change in place is uploaded again"""
    ctx, other = pa.Context(0, lib), pa.Context(0, lib)
    dc.clear_upload_cache()
    X = explicit_matrix(4, 6, 71, lambda i, j: True)
    dX = pa.DeviceCsr.from_scipy(X, ctx)
    P = sps.csr_matrix((np.ones(4), np.array([1, 0, 3, 2], dtype=np.int32), np.arange(5, dtype=np.int32)), shape=(4, 4))
    d1 = pa.DeviceCsr.from_any(P, ctx)
    same((d1 @ dX).to_scipy(), P @ X)
    assert pa.DeviceCsr.from_any(P, ctx) is d1          # unchanged: served from the cache
    assert (P @ dX) is not None and pa.DeviceCsr.from_any(P, ctx) is d1   # (the operator route takes the same entry)
    P.indices[:] = [3, 2, 1, 0]                          # same shape, nnz and values
    d2 = pa.DeviceCsr.from_any(P, ctx)
    assert d2 is not d1
    same((d2 @ dX).to_scipy(), X[::-1])
    same((P @ dX).to_scipy(), X[::-1])
    P.data[2] = 2.0                                      # one value
    d3 = pa.DeviceCsr.from_any(P, ctx)
    assert d3 is not d2
    same(d3.to_scipy(), P)
    Q = sps.csr_matrix((np.ones(4), np.array([0, 1, 2, 3], dtype=np.int32), np.array([0, 1, 2, 3, 4], dtype=np.int32)), shape=(4, 4))
    q1 = pa.DeviceCsr.from_any(Q, ctx)
    Q.indptr[:] = [0, 0, 2, 4, 4]                        # same nnz, indices and values: rows 1 and 2 take two entries each
    q2 = pa.DeviceCsr.from_any(Q, ctx)
    assert q2 is not q1
    same(q2.to_scipy(), sps.csr_matrix((Q.data, Q.indices, Q.indptr), shape=(4, 4)))
    assert pa.DeviceCsr.from_any(Q, ctx) is q2
    o1 = pa.DeviceCsr.from_any(Q, other)                 # another handle: its own copy
    assert o1 is not q2 and o1.ctx is other
    same(o1.to_scipy(), q2.to_scipy())
    q3 = pa.DeviceCsr.from_any(Q, ctx)                   # (the entry now belongs to the other handle: uploaded again)
    assert q3 is not o1 and q3.ctx is ctx
    assert pa.DeviceCsr.from_any(Q, ctx) is q3
    pa.DeviceCsr.invalidate(Q)
    q4 = pa.DeviceCsr.from_any(Q, ctx)
    assert q4 is not q3 and pa.DeviceCsr.from_any(Q, ctx) is q4
    dc.clear_upload_cache()
    q5 = pa.DeviceCsr.from_any(Q, ctx)
    assert q5 is not q4 and pa.DeviceCsr.from_any(Q, ctx) is q5
    dc.clear_upload_cache()
    ctx.close()
    other.close()


# --------------------------------------------------------------------------------------------------- C ABI input checks
def from_host(ctx, nrows, ncols, indptr, indices, data):
    ip, ix = np.asarray(indptr, dtype=np.int32), np.asarray(indices, dtype=np.int32)
    dv = np.asarray(data, dtype=np.float64)
    out = _lib._h()
    st = ctx.lib.pfv_csr_from_host(ctx._h, nrows, ncols, _lib._ptr(ip, _lib._ip), _lib._ptr(ix, _lib._ip),
                                   _lib._ptr(dv, _lib._dp), ctypes.byref(out))
    msg = ctx.lib.pfv_last_error(ctx._h).decode(errors="replace") if st else ""
    if st == 0:
        ctx.lib.pfv_csr_free(out)
    return st, msg


ERR_ARGUMENT = 4


def abi_rows_are_checked(lib, monkeypatch, hooks):
    """pfv_csr_from_host refuses a duplicate column, an index equal to ncols and a negative index (every index read lies
    inside the uploaded arrays); the handle works afterwards"""
    ctx = pa.Context(0, lib)
    for indices in ([1, 1, 3], [0, 2, 5], [-1, 2, 4]):
        st, msg = from_host(ctx, 2, 5, [0, 2, 3], indices, [1.0, 2.0, 3.0])
        assert st == ERR_ARGUMENT and "sorted by column" in msg
    st, _ = from_host(ctx, 2, 5, [0, 2, 3], [0, 4, 4], [1.0, 2.0, 3.0])
    assert st == 0
    st, msg = from_host(ctx, 2, 5, [1, 2, 3], [0, 4, 4], [1.0, 2.0, 3.0])
    assert st == ERR_ARGUMENT and "bad matrix" in msg
    ctx.close()


def abi_indptr_is_checked_on_the_host(lib, monkeypatch, hooks):
    """A decreasing indptr ([0, 5, 2] with two stored entries) and an indptr entry above nnz ([0, 3, 2]) are refused by the
    walk over indptr on the host, with a message of their own, before anything is uploaded or launched.

    EMULATION BUILD ONLY.  These two inputs are not in the GPU suite: were the host check missing, the row check on the
    device would read indices[e] for e in [indptr[r], indptr[r + 1]) -- outside the two-element buffer -- before
    anything is refused.  A machine that others share is not the place to find that out; the check is host code, the
    same in both builds, and the emulation build runs it."""
    ctx = pa.Context(0, lib)
    assert not ctx.lib.pfv_is_device_build()
    for indptr in ([0, 5, 2], [0, 3, 2], [0, -1, 2]):
        st, msg = from_host(ctx, 2, 5, indptr, [1, 3], [1.0, 2.0])
        assert st == ERR_ARGUMENT and "indptr must be non-decreasing and within [0, nnz]" in msg, (indptr, st, msg)
    st, _ = from_host(ctx, 2, 5, [0, 2, 2], [1, 3], [1.0, 2.0])
    assert st == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ the lists
def _case(fn, *args):
    return pytest.param(fn, args, id="-".join([fn.__name__] + [str(a) for a in args]))


CASES = (
    [_case(product_class_edge, m) for m in EDGE_COUNTS]
    + [_case(product_4096_forced_and_4097)]
    + [_case(product_mixed_rows, lanes, n) for lanes in (16, 32, 64) for n in (1, 3, 4, 5, "all")]
    + [_case(product_second_grid_trip, lanes) for lanes in (16, 32, 64)]
    + [_case(product_keep_mask, name) for name in KEEP_MASK_PAIRS]
    + [_case(product_keys), _case(product_generic_empty)]
    + [_case(product_generic_key_bits, ncols, n) for ncols in (1, 2, 3, 2 ** 16, 2 ** 16 + 1) for n in (1, 2, 3)]
    + [_case(transpose_widths, ncols) for ncols in (1, 2, 3, 64, 65, 2 ** 16, 2 ** 16 + 1)]
    + [_case(transpose_empty), _case(sum_cases), _case(block_cases), _case(operator_row_selection),
       _case(operator_division), _case(operator_scipy_operands), _case(operator_device_vectors),
       _case(routes_to_the_solver), _case(upload_cache), _case(abi_rows_are_checked)]
)
EMULATION_ONLY = [_case(abi_indptr_is_checked_on_the_host)]
