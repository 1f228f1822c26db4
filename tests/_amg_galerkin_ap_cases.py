"""Cases of the first coarse operator formed from AP = A_s P (PFV_AMG_GALERKIN_AP; csrc/amg.inc: amg_coarsen_level,
amg_build_ap), shared by the emulation suite (test_amg_galerkin_ap_emulation.py) and the GPU suite
(test_gpu_amg_galerkin_ap.py).

On kept aggregate maps level 1 is one Galerkin product P^T (A_s P) over the double-precision sums of AP instead of the
three pairwise products over A_s.  The route needs AP, which small systems only build under PFV_AMG_FUSE_ROWS=0 (as in
tests/_amg_ap_cases.py), and kept maps: every case sets up once (cold: the passes), moves the values on the same pattern
and sets up again.  ``stats()["amg_galerkin_ap"]`` tells which route the last setup took.

The route is judged like every other: check_setup / check_cycle of tests/_amg_cases.py on its own read-out (Galerkin
identity against a long-double P^T A P, bound = FACTOR x the float64-vs-longdouble difference of the case), and against
the pass route on the same values with hierarchies_equal: maps and patterns bitwise, values within the larger of the
two cycle bounds (the routes differ by the order of the additions only)."""
import numpy as np
import scipy.sparse as sps

import porepy_amd as pa
from tests import _amg_ap_cases as AP
from tests import _amg_cases as C

LD = np.longdouble
BASE = {"PFV_AMG_FUSE_ROWS": "0"}
SWITCH = "PFV_AMG_GALERKIN_AP"


def route(ctx):
    return int(ctx.stats()["amg_galerkin_ap"])


def ap_inputs(H0):
    """Entries that feed every coarse row through AP: the distinct aggregates among the columns of its member rows."""
    op, agg = H0["op"], H0["agg"]
    n = op.shape[0]
    S = sps.csr_matrix((np.ones(op.nnz), op.indices, op.indptr), shape=op.shape)
    Pm = sps.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, int(agg.max()) + 1))
    return np.bincount(agg, weights=np.diff((S @ Pm).tocsr().indptr), minlength=int(agg.max()) + 1).astype(np.int64)


def move_flow(S, rng, sigma=0.3):
    """Cell-wise random factors on the permeability: the values move, and with them the filtered pattern."""
    S.set_values(S.sc * np.exp(sigma * rng.standard_normal(S.g.num_cells)))


def move_user(S, rng, sigma=0.05):
    """F A F with a random positive diagonal F close to one: same pattern, every value moves."""
    f = np.exp(sigma * rng.standard_normal(S.n))
    A = sps.csr_matrix(S.A)
    row = C.row_of_entries(A)
    B = sps.csr_matrix((A.data * f[row] * f[A.indices], A.indices.copy(), A.indptr.copy()), shape=A.shape)
    S.A = B
    S.ctx.set_system(B, S.b)


def setup(S, lib, env, want_route, want_reused, check=True, V=None):
    with C.environment(env):
        S.ctx.amg_setup(0)
        H = C.read_hierarchy(S.ctx)
        got = route(S.ctx)
        if got:  # (built before the product now: still the AP the cycle is entitled to)
            assert int(S.ctx.stats()["amg_ap_nnz"]) == AP.ap_entries(H[0])
        assert H[0]["reused"] == want_reused, ("reused", H[0]["reused"], env)
        assert got == want_route, ("route", got, want_route, env)
        out = {"H": H, "route": got}
        if check:
            out["setup"] = C.check_setup(H)
            out["V"] = C.case_vectors(H, 3) if V is None else V
            out["cycle"] = C.check_cycle(S.ctx, lib, H, V=out["V"])
    return out


def kept_against_passes(S, lib, env=None, expect=None, V=None):
    """On a handle in the kept state: the pass route, then the route from AP, on the same values."""
    env = dict(BASE, **(env or {}))
    off = setup(S, lib, dict(env, **{SWITCH: "0"}), 0, True, V=V)
    on = setup(S, lib, dict(env, **{SWITCH: "1"}), 1, True, V=off["V"])
    if expect is not None:
        expect(on["H"])
    tol = max(on["cycle"]["bound"], off["cycle"]["bound"])
    C.hierarchies_equal(off["H"], on["H"], tol)
    diff = C.max_rel(on["cycle"]["Z"], off["cycle"]["Z"].astype(LD))
    inp = ap_inputs(on["H"][0])
    a, b = off["H"][1]["A"], on["H"][1]["A"]
    vdiff = float(np.max(np.abs(a.data - b.data)) / np.max(np.abs(a.data)))
    print(f"galerkin_ap on/off: rows {[h['n'] for h in on['H']]} inputs per coarse row min {inp.min()} "
          f"median {int(np.median(inp))} max {inp.max()} (gathered max {on['H'][0]['galerkin_max_gather']}) "
          f"level-1 values on-off {vdiff:.2e} galerkin err {on['setup']['galerkin'][0][2]:.2e} "
          f"bound {on['setup']['galerkin'][0][1]:.2e} cycle on-off {diff:.2e} bound {tol:.2e}")
    assert diff <= tol, ("on against off", diff, tol)
    # the product that was sized last setup is the one over AP
    assert on["H"][0]["galerkin_max_gather"] >= inp.max()
    return on, off


def case(make_system, move, lib, env=None, expect=None, seed=31):
    """Cold setup (the passes, and it says so), moved values, then the two routes on the kept maps."""
    S = make_system()
    rng = np.random.default_rng(seed)
    cold = setup(S, lib, dict(BASE, **(env or {}), **{SWITCH: "1"}), 0, False, check=False)
    move(S, rng)
    on, off = kept_against_passes(S, lib, env, expect)
    for a, b in zip(cold["H"][:-1], on["H"][:-1]):
        assert np.array_equal(a["agg"], b["agg"])  # kept maps
    assert not np.array_equal(cold["H"][1]["A"].data, on["H"][1]["A"].data)  # ... and moved values
    return on, off


def both_sides_of_64(H):
    inp = ap_inputs(H[0])
    assert inp.min() <= 64 < inp.max(), (inp.min(), inp.max())


def tets(lib, gamma, n=8):
    def expect(H):
        assert H[0]["n"] == 6 * n ** 3 and len(H) >= 3 and H[0]["gamma"] == gamma
        assert ("second_visit" in H[0]["path"]) == (gamma == 2)
        both_sides_of_64(H)
    return case(lambda: C.FlowSystem(lib, C.tet_grid(n), seed=4), move_flow, lib, {"PFV_AMG_GAMMA": str(gamma)}, expect)


def cartesian_3d(lib, n=24):
    def expect(H):
        assert H[0]["n"] == n ** 3 and len(H) >= 3
        both_sides_of_64(H)
    return case(lambda: C.FlowSystem(lib, C.cart_grid([n, n, n]), seed=5, sigma=1.0), move_flow, lib, expect=expect)


def long_rows(lib):
    """A hub row of several hundred entries: the one-lane insertion of the ranking carries the double sums too, and the
    hub's coarse row gathers more than the batched gather holds (member by member for the whole product)."""
    A, hub = C.edge_case_matrix(n=8000, hub_degree=1500)  # (enough aggregates for the hub to reach 512 distinct ones)

    def expect(H):
        assert np.diff(H[0]["op"].indptr)[hub] > 128
        assert ap_inputs(H[0]).max() > H[0]["gal_epl"] * 64
        assert np.bincount(H[0]["agg"]).max() > H[0]["gal_max_members"]
    return case(lambda: C.UserSystem(lib, A), move_user, lib, expect=expect)


def wide_coarse_rows(lib):
    """Coarse rows of more than 160 inputs that the batched gather still holds: the 64-lane group."""
    A, hub = C.edge_case_matrix(n=5000, hub_degree=400)

    def expect(H):
        assert np.diff(H[0]["op"].indptr)[hub] > 128
        assert 160 < ap_inputs(H[0]).max() <= H[0]["gal_epl"] * 64
    return case(lambda: C.UserSystem(lib, A), move_user, lib, expect=expect)


def star_matrix(n=1200, leaves=40, seed=13):
    """The graph system with one centre whose `leaves` neighbours have no other strong coupling: they all join the
    centre's pair, an aggregate of more members than the batched gather takes."""
    rng = np.random.default_rng(seed)
    A = C.graph_matrix(n, rng).tolil()
    centre = 5
    A.resize((n + leaves, n + leaves))
    for k in range(leaves):
        j = n + k
        w = 50.0 * (1 + rng.random())
        A[centre, j] = -w
        A[j, centre] = -w
        A[centre, centre] += 1.05 * w
        A[j, j] = 1.05 * w
    return C.shuffled_columns(A.tocsr(), rng), centre


def many_members(lib):
    A, centre = star_matrix()

    def expect(H):
        sizes = np.bincount(H[0]["agg"])
        assert sizes[H[0]["agg"][centre]] > H[0]["gal_max_members"], sizes.max()
    return case(lambda: C.UserSystem(lib, A), move_user, lib, expect=expect)


def without_locality(lib):
    def expect(H):
        assert H[0]["op"].nnz >= 200000 and not H[0]["window"] and len(H) == 2
        assert C.window_columns(H[0]["op"]) > 4096
    return case(lambda: C.UserSystem(lib, C.no_locality_matrix()), move_user, lib, {"PFV_AMG_COARSE_TARGET": "1024"},
                expect=expect)


# ---------------------------------------------------------------------------------------------------------------------
# fallbacks: the pass route, and the setup says so

def fallback_switch(lib, env, n=8):
    """Kept maps under a switch that rules the route out."""
    S = C.FlowSystem(lib, C.tet_grid(n), seed=4)
    env = dict(BASE, **env)
    setup(S, lib, env, 0, False, check=False)
    move_flow(S, np.random.default_rng(2))
    return setup(S, lib, env, 0, True)


def fallback_block_system(lib):
    S = C.MechSystem(lib, C.tet_grid(5))
    setup(S, lib, BASE, 0, False, check=False)
    out = setup(S, lib, BASE, 0, True)
    assert out["H"][0]["block_size"] == 3
    return out


def fallback_cold_and_switch_change(lib, n=8):
    """The first setup and a setup after a change of a matching switch re-match: the passes.  Between them and after
    them the kept state takes the route from AP."""
    S = C.FlowSystem(lib, C.tet_grid(n), seed=4)
    rng = np.random.default_rng(6)
    setup(S, lib, BASE, 0, False)
    move_flow(S, rng)
    setup(S, lib, BASE, 1, True, check=False)
    changed = dict(BASE, PFV_AMG_ROUNDS="1")
    setup(S, lib, changed, 0, False)
    setup(S, lib, changed, 1, True)
    setup(S, lib, BASE, 0, False)
    return setup(S, lib, BASE, 1, True)


def fallback_different_pattern(lib, n=900, seed=12):
    """Equal rows and entries, another pattern, on one handle: re-matched by the passes, then kept."""
    rng = np.random.default_rng(seed)
    A = C.graph_matrix(n, rng)
    A.sort_indices()
    perm = rng.permutation(n)
    B = sps.csr_matrix(A[perm][:, perm])
    assert B.nnz == A.nnz and not np.array_equal(A.indices, B.indices)
    S = C.UserSystem(lib, A)
    setup(S, lib, BASE, 0, False, check=False)
    S.ctx.set_system(A, S.b)
    setup(S, lib, BASE, 1, True)
    S.A = B
    S.ctx.set_system(B, S.b)
    setup(S, lib, BASE, 0, False)
    S.ctx.set_system(B, S.b)
    return setup(S, lib, BASE, 1, True)


# ---------------------------------------------------------------------------------------------------------------------
# state

def level1_bits(H):
    return [(h["A"].indptr.copy(), h["A"].indices.copy(), h["A"].data.copy(), h["dinv"].copy()) for h in H[1:]]


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for la, lb in zip(a, b) for x, y in zip(la, lb))


def state_sequence(lib, n=8):
    """Cold -> kept -> kept on moving values, then the switch flipped 1 -> 0 -> 1 on the same values: every kept
    hierarchy equals the pass-route hierarchy of the values on the handle (a stale size record or stale double sums of
    AP would not), and the route gives the same bits whenever it is taken on the same values."""
    S = C.FlowSystem(lib, C.tet_grid(n), seed=4)
    rng = np.random.default_rng(17)
    on = dict(BASE, **{SWITCH: "1"})
    off = dict(BASE, **{SWITCH: "0"})
    setup(S, lib, on, 0, False)
    seen = []
    for step in range(2):
        move_flow(S, rng, 0.3 + 0.5 * step)  # (the second move is large enough for the filter to keep other entries)
        a = setup(S, lib, on, 1, True)
        assert abs(a["H"][0]["sys"] - S.A).max() == 0.0  # the hierarchy belongs to the values on the handle NOW
        seen.append(a)
    assert not np.array_equal(seen[0]["H"][0]["A"].indptr, seen[1]["H"][0]["A"].indptr), "the filter kept the same entries"
    assert not same_bits(level1_bits(seen[0]["H"]), level1_bits(seen[1]["H"]))
    b = setup(S, lib, off, 0, True, V=seen[1]["V"])
    c = setup(S, lib, on, 1, True, V=seen[1]["V"])
    for x in (seen[1], c):
        C.hierarchies_equal(b["H"], x["H"], max(b["cycle"]["bound"], x["cycle"]["bound"]))
    assert same_bits(level1_bits(seen[1]["H"]), level1_bits(c["H"])), "the route from AP differs after the passes ran"
    # the previous values' level-1 matrix must not pass for the new ones
    try:
        C.check_galerkin(c["H"][0], seen[0]["H"][1])
    except AssertionError:
        pass
    else:
        raise AssertionError("a stale level-1 matrix passes the Galerkin check")
    return seen + [b, c]


def determinism(lib, n=8):
    """Two kept setups on identical values: level 1 and everything below it, and the applied cycle, bit for bit."""
    S = C.FlowSystem(lib, C.tet_grid(n), seed=4)
    env = dict(BASE, **{SWITCH: "1", "PFV_AMG_GAMMA": "2"})
    setup(S, lib, env, 0, False, check=False)
    move_flow(S, np.random.default_rng(3))
    a = setup(S, lib, env, 1, True, check=False)
    with C.environment(env):
        V = C.case_vectors(a["H"], 3)
        Z1 = C.apply_cycle(S.ctx, lib, V)
    b = setup(S, lib, env, 1, True, check=False)
    with C.environment(env):
        Z2 = C.apply_cycle(S.ctx, lib, V)
    assert same_bits(level1_bits(a["H"]), level1_bits(b["H"])), "two setups from the same values differ"
    assert np.array_equal(Z1, Z2)
    return True


def solve_route_against_passes(lib, g, rtol=1e-12):
    """BiCGStab + AMG by the criteria of _amg_ap_cases.solve_on_against_off, between the two routes: a first solve
    (cold), new permeabilities, and the solve on the kept maps -- iterations within 1, solutions to 1e-9 relative."""
    rng = np.random.default_rng(4)
    sc0 = np.exp(0.5 * rng.standard_normal(g.num_cells))
    sc1 = sc0 * np.exp(0.3 * rng.standard_normal(g.num_cells))

    def tensor(sc):
        kw = dict(kxx=sc, kyy=3 * sc, kxy=0.3 * sc)
        if g.dim == 3:
            kw.update(kzz=0.4 * sc, kyz=0.1 * sc)
        return pa.SecondOrderTensor(**kw)
    bf = g.get_all_boundary_faces()
    xf = g.face_centers[0, bf]
    dirf = bf[(xf < 1e-9) | (xf > g.nodes[0].max() - 1e-9)]
    bv = np.zeros(g.num_faces)
    bv[dirf] = g.face_centers[0, dirf]
    res = {}
    for sw in ("0", "1"):
        with C.environment(dict(BASE, **{SWITCH: sw, "PFV_AMG_GAMMA": "2"})):
            data = pa.initialize_data({}, "flow", {"second_order_tensor": tensor(sc0),
                                                   "bc": pa.BoundaryCondition(g, dirf, ["dir"] * dirf.size),
                                                   "bc_values": bv})
            d = pa.Mpfa("flow", library=lib)
            for k, sc in enumerate((sc0, sc1)):
                data[pa.PARAMETERS]["flow"]["second_order_tensor"] = tensor(sc)
                d.discretize(g, data)
                d.assemble_matrix_rhs(g, data)
                x, info = d.solve(g, data, source=g.cell_volumes, method="bicgstab", rtol=rtol, precond="amg")
                assert info["converged"], (sw, k, info)
                st = d.context(g).stats()
                assert int(st["amg_galerkin_ap"]) == (1 if (k == 1 and sw == "1") else 0), (sw, k)
                assert int(st["amg_maps_reused"]) == k
            res[sw] = (x, int(info["iterations"]), int(st["amg_levels"]))
            d.context(g).close()
    (x0, it0, lev), (x1, it1, _) = res["0"], res["1"]
    print(f"galerkin_ap solve on kept maps: iterations passes {it0} from AP {it1}")
    assert lev >= 3
    assert abs(it1 - it0) <= 1, (it0, it1)
    assert np.linalg.norm(x1 - x0) <= 1e-9 * np.linalg.norm(x0)
    return it0, it1
