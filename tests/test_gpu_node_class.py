"""GPU suite (-m gpu): the interaction-region bodies at every class edge and on the redo path.

The device picks the body of a node by the number n of faces that meet in it: launch_node_class<8>, <16>, <32>, <64,40>,
<64,48>, <64,64> and the LDS Gauss-Jordan beyond 64 for MPFA (csrc/mpfa_numeric.inc), the register elimination up to
nd n = 128 unknowns and the LDS / global-scratch one beyond for MPSA (csrc/mpsa.inc).  The classes 32 < n <= 48 (MPFA) and
nd n <= 128 (MPSA) eliminate without a pivot search, verify, and hand what fails to a redo list.  None of this is in the
host-emulation build.  The fans of tests/_node_class_cases.py put a node on either side of each edge; the redo path is
run by setting the acceptance tolerance to 0 (PFV_NODE_NP_TOLX / PFV_MPSA_NP_TOLX), on regular problems that the
emulation suite has already checked against the oracle (tests/test_node_class_emulation.py)."""
import pytest

import porepy_amd as pa
from tests import _node_class_cases as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()  # raises if the HIP build is missing


# ---------------------------------------------------------------------------- a. every class edge, default switches
@pytest.mark.parametrize("n", N.MPFA_EDGES)
def test_mpfa_class_edge(lib, monkeypatch, n):
    p = N.problem("mpfa", n)
    mats, redo = N.run(lib, p, monkeypatch)
    print(f"mpfa n={n}: node_redo {redo}")
    N.assert_oracle(p, mats, f"n={n}")
    assert 0 <= redo <= N.count_between(p.g, 32, 48)


@pytest.mark.parametrize("n", N.MPSA_EDGES)
def test_mpsa_class_edge(lib, monkeypatch, n):
    p = N.problem("mpsa", n)
    mats, redo = N.run(lib, p, monkeypatch)
    print(f"mpsa n={n}: node_redo {redo}")
    N.assert_oracle(p, mats, f"n={n}")
    assert 0 <= redo <= p.g.num_nodes


# ---------------------------------------------------------------------- b. the optimistic path is really the default
def test_mpfa_benchmark_like_lattice_redoes_nothing(lib, monkeypatch):
    p = N.problem("mpfa", "lattice")
    assert N.count_between(p.g, 32, 48) == 27  # (the interior nodes, n = 36: the unpivoted class)
    mats, redo = N.run(lib, p, monkeypatch)
    assert redo == 0  # (no region of the benchmark fails the check)
    N.assert_oracle(p, mats, "lattice, default")
    mats3, redo3 = N.run(lib, p, monkeypatch, {"PFV_NODE_GJ": 3})
    assert redo3 == 0
    N.assert_oracle(p, mats3, "lattice, PFV_NODE_GJ=3")


# -------------------------------------------------------------------------------------------- c. forced redo, MPFA
@pytest.mark.parametrize("name", [36, 44, (36, 44), "lattice"], ids=str)
def test_mpfa_forced_redo_takes_every_optimistic_node(lib, monkeypatch, name):
    p = N.problem("mpfa", name)
    mats, redo = N.run(lib, p, monkeypatch, {"PFV_NODE_NP_TOLX": 0})
    assert redo == N.count_between(p.g, 32, 48) > 0
    N.assert_oracle(p, mats, f"{name}, forced redo")


@pytest.mark.parametrize("n", [32, 33, 40, 41, 48, 49])
def test_mpfa_forced_redo_at_the_edges_of_the_optimistic_classes(lib, monkeypatch, n):
    """32 < n <= 48 exactly: hub and pole of the fans 33 ... 48 are redone, those of 32 and 49 never are."""
    p = N.problem("mpfa", n)
    mats, redo = N.run(lib, p, monkeypatch, {"PFV_NODE_NP_TOLX": 0})
    assert redo == (2 if 32 < n <= 48 else 0)
    N.assert_oracle(p, mats, f"n={n}, forced redo")


@pytest.mark.parametrize("n", [36, 44])
def test_mpfa_forced_redo_is_the_pivoted_body(lib, monkeypatch, n):
    """One optimistic class in the grid: the redo launch is the node_gj_reg2d instantiation PFV_NODE_GJ=3 runs."""
    p = N.problem("mpfa", n)
    forced, _ = N.run(lib, p, monkeypatch, {"PFV_NODE_NP_TOLX": 0})
    pivoted, redo3 = N.run(lib, p, monkeypatch, {"PFV_NODE_GJ": 3})
    assert redo3 == 0
    assert N.same_bits(forced, pivoted)


@pytest.mark.parametrize("name", [36, (36, 44), "lattice"], ids=str)
def test_mpfa_redo_leaves_no_state_behind(lib, monkeypatch, name):
    """Same handle: default, forced, forced, default.  The forced runs agree bit for bit (the order of the redo list comes
    from an atomic counter), and the default run afterwards counts and computes what it did before."""
    p = N.problem("mpfa", name)
    ctx = N.open_context(lib, p)
    try:
        d0, r0 = N.discretize(ctx, p, monkeypatch)
        f1, q1 = N.discretize(ctx, p, monkeypatch, {"PFV_NODE_NP_TOLX": 0})
        f2, q2 = N.discretize(ctx, p, monkeypatch, {"PFV_NODE_NP_TOLX": 0})
        d1, r1 = N.discretize(ctx, p, monkeypatch)
    finally:
        ctx.close()
    assert q1 == q2 == N.count_between(p.g, 32, 48)
    assert N.same_bits(f1, f2)
    assert r1 == r0 and N.same_bits(d0, d1)
    N.assert_oracle(p, d1, f"{name}, default after forced")


# -------------------------------------------------------------------------------------------- d. forced redo, MPSA
@pytest.mark.parametrize("name", [36, (36, 44), 42, 43], ids=str)
def test_mpsa_forced_redo_wide_and_fp64(lib, monkeypatch, name):
    """(42 | 43: the last fan whose hubs take the unpivoted register elimination, 126 unknowns, and the first that do not)"""
    p = N.problem("mpsa", name)
    small = N.count_between(p.g, 0, 128, scale=3)
    assert small >= p.g.num_nodes - 2 * (len(name) if isinstance(name, tuple) else 1)
    for wide in (1, 0):
        mats, redo = N.run(lib, p, monkeypatch, {"PFV_MPSA_NP_TOLX": 0, "PFV_MPSA_REDO_WIDE": wide})
        print(f"mpsa {name}: REDO_WIDE={wide} node_redo {redo} (nodes with nd n <= 128: {small} of {p.g.num_nodes})")
        assert small <= redo <= p.g.num_nodes
        N.assert_oracle(p, mats, f"{name}, forced redo, REDO_WIDE={wide}")
    mats, _ = N.run(lib, p, monkeypatch, {"PFV_MPSA_GJ_NP": 0})
    N.assert_oracle(p, mats, f"{name}, PFV_MPSA_GJ_NP=0")


@pytest.mark.parametrize("name", [36, (36, 44)], ids=str)
def test_mpsa_pivoted_register_body_redoes_what_the_default_redoes(lib, monkeypatch, name):
    p = N.problem("mpsa", name)
    _, base = N.run(lib, p, monkeypatch)
    mats, redo = N.run(lib, p, monkeypatch, {"PFV_MPSA_GJ_NP": 0})
    print(f"mpsa {name}: node_redo {base} by default, {redo} with PFV_MPSA_GJ_NP=0")
    N.assert_oracle(p, mats, f"{name}, PFV_MPSA_GJ_NP=0")
    assert redo == base


def test_mpsa_forced_redo_beyond_the_count_keeps_the_fp64_body(lib, monkeypatch):
    """2 116 nodes > max(2000, nn / 50): the wide body is asked for and the FP64 body runs -- the bits say which."""
    p = N.problem("mpsa", "tri45")
    assert p.g.num_nodes == 2116
    wide, redo_w = N.run(lib, p, monkeypatch, {"PFV_MPSA_NP_TOLX": 0, "PFV_MPSA_REDO_WIDE": 1})
    assert redo_w == 2116
    N.assert_oracle(p, wide, "45 x 45 triangles, forced redo")
    fp64, redo_f = N.run(lib, p, monkeypatch, {"PFV_MPSA_NP_TOLX": 0, "PFV_MPSA_REDO_WIDE": 0})
    assert redo_f == 2116
    assert N.same_bits(wide, fp64)


def test_mpsa_systems_smaller_than_the_exchange_buffers_pass_the_check(lib, monkeypatch):
    """Every region of a 2-D grid has n <= 22 unknowns, less than the 512 doubles mpsa_gj_reg_np exchanges through L.A: with
    L.A sized by n * ld alone the buffers ran over the arrays behind it, the check never passed and all 2 116 regions were
    computed twice (the same 2 116 whether the tolerance was 1 or 1e9 times the default).  A regular structured grid is no
    input "on which the unpivoted elimination fails its check everywhere": at most the nn / 50 that mpsa.inc itself takes
    for the limit of that (the count branch of the redo launch)."""
    p = N.problem("mpsa", "tri45")
    mats, redo = N.run(lib, p, monkeypatch)
    print(f"mpsa 45 x 45 triangles, default: node_redo {redo} of {p.g.num_nodes}")
    N.assert_oracle(p, mats, "45 x 45 triangles, default")
    assert redo <= p.g.num_nodes // 50


# ------------------------------------------------------------------------ e. default bits unchanged by the new switch
@pytest.mark.parametrize("name", [36, "lattice"], ids=str)
def test_mpfa_tolerance_switch_at_one_is_the_default(lib, monkeypatch, name):
    p = N.problem("mpfa", name)
    unset, r0 = N.run(lib, p, monkeypatch)
    one, r1 = N.run(lib, p, monkeypatch, {"PFV_NODE_NP_TOLX": 1})
    assert r0 == r1 and N.same_bits(unset, one)


# -------------------------------------------------------------------------- f. partial update through the redo path
def test_mpfa_partial_update_through_redo(lib, monkeypatch):
    N.partial_update_through_redo(lib, monkeypatch, expect_redo=2)
