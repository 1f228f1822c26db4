"""The cases of tests/test_gpu_node_class.py on the host-emulation build: the fans are regular problems (every matrix
within TOL of the oracle, patterns index for index), and the helpers, boundary conditions and tensors are right -- shown
here before any of them reaches a GPU.  The emulation takes the LDS Gauss-Jordan for every region: the
register bodies, the unpivoted elimination and the redo hand-over are pinned by the GPU file alone."""
import numpy as np
import pytest

from tests import _node_class_cases as N
from tests import _parity as P


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


@pytest.mark.parametrize("n", (5, 6, 8, 9, 32, 33, 41, 64, 65, 129))
def test_fan_has_exactly_n_faces_at_hub_and_pole(n):
    g = N.fan_grid_3d(n)  # (asserts the count itself)
    cnt = N.faces_per_node(g)
    assert cnt[0] == n and cnt[1] == n and cnt[2:].max() <= 6
    assert g.num_cells == (n // 2 if n % 2 == 0 else (n + 1) // 2 - 1)
    assert np.all(g.cell_volumes > 0)


def test_union_has_the_hubs_of_both_fans():
    g = N.fan_union_3d((36, 44))
    cnt = N.faces_per_node(g)
    (h0, p0), (h1, p1) = g.fan_hubs
    assert [cnt[h0], cnt[p0], cnt[h1], cnt[p1]] == [36, 36, 44, 44]
    assert N.count_between(g, 32, 40) == 2 and N.count_between(g, 40, 48) == 2 and N.count_between(g, 32, 48) == 4
    assert g.num_cells == 18 + 22 and np.intersect1d(g.fan_cells[0], g.fan_cells[1]).size == 0
    assert N.count_between(N.lattice_grid(), 32, 48) == 27  # (the interior nodes of the 4^3 Kuhn lattice: n = 36)


@pytest.mark.parametrize("n", N.MPFA_EDGES)
def test_mpfa_fan_against_oracle(lib, n):
    assert N.check_against_oracle(lib, "mpfa", n) == 0  # (no unpivoted elimination in this build: nothing to redo)


@pytest.mark.parametrize("n", N.MPSA_EDGES)
def test_mpsa_fan_against_oracle(lib, n):
    N.check_against_oracle(lib, "mpsa", n)


@pytest.mark.parametrize("kind, name", [("mpfa", 36), ("mpfa", 44), ("mpfa", (36, 44)), ("mpfa", "lattice"),
                                        ("mpsa", 36), ("mpsa", (36, 44)), ("mpsa", "tri45")])
def test_inputs_of_the_forced_redo_cases_are_regular(lib, kind, name):
    N.check_against_oracle(lib, kind, name)


def test_partial_update_case_on_the_union(lib, monkeypatch):
    N.partial_update_through_redo(lib, monkeypatch, expect_redo=0)
