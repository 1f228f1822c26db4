"""CPU suite for the SpMV family on the host-emulation build (only the plain product exists there: no windows, no lane
trees) and the self-checks of the references every case of tests/_spmv_cases.py is judged by; tests/test_gpu_spmv.py
runs the same cases on the HIP library, where the windowed and the fused-dot kernels live."""
import numpy as np
import pytest

from tests import _parity as P
from tests import _spmv_cases as C


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


# ---- the references themselves ----------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [8, 16, 32])
def test_exact_reference_is_exact(lanes):
    C.exact_reference_self_check(C.ladder_case(lanes))
    C.exact_reference_self_check(C.ladder_case(lanes, dup=True))


@pytest.mark.parametrize("lanes", [8, 16, 32])
def test_bound_holds_for_float64_products_and_is_not_vacuous(lanes):
    C.bound_is_not_vacuous(C.ladder_case(lanes))


def test_bound_on_the_other_patterns():
    for case in (C.Case("row view", C.view_pattern()), C.Case("tails n129", C.tail_pattern(129)),
                 C.builder_case(1025)):
        if case.n <= 1000:
            C.bound_is_not_vacuous(case)
        A, x = case.bounded
        yhat, bound = C.bounded_reference(A, x)
        assert np.all(np.abs((A @ x).astype(C.LD) - yhat) <= bound), case.name


def test_builder_patterns_hold_what_the_issue_asks():
    for w in C.BUILDER_W:
        case = C.builder_case(w)  # (asserts exactly W distinct columns in block 0, W the largest window)
        A = case.exact[0]
        head = np.unique(A.indices[: A.indptr[C.WIN_ROWS]])
        assert head[0] == 0 and head[-1] == C.BUILDER_N - 1
        assert np.all(np.isin(np.arange(C.WIN_ROWS, C.BUILDER_N, 8192), head))  # a run spaced by the table size
        crowd = C.win_hash(head) >= 8192 - 200
        assert crowd.sum() >= w - 400  # the rest piles onto the last 200 slots of the 8192-slot table
        assert np.all(A.indices[A.indptr[C.WIN_ROWS]:] == np.arange(C.WIN_ROWS, C.BUILDER_N))


@pytest.mark.parametrize("name,method", C.KRYLOV_RUNS)
def test_krylov_restatement_noise(name, method):
    """the restatement converges on its own terms (one iteration reduces the residual) and its float64 spread, which the
    tolerance of the one-iteration tests is 8 times of, is at the rounding level of a dot product of length n"""
    A, b, lanes, ref, noise, allowed = C.krylov_reference(name, method)
    print("one %s iteration, %s: noise %.3e allowed %.3e" % (method, name, noise, allowed))
    assert allowed == 8.0 * noise and 1e-18 < noise <= 16 * A.shape[0] * C.UNIT
    r1 = b - A @ np.asarray(ref, dtype=np.float64)
    assert np.linalg.norm(r1) < np.linalg.norm(b)


# ---- the cases on the emulation library --------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [8, 16, 32])
def test_ladder_products(lib, lanes):
    C.ladder_products(lib, lanes)


@pytest.mark.parametrize("n", C.TAIL_SIZES)
def test_block_and_pass_tails(lib, n):
    C.tail_products(lib, n)


def test_row_view(lib):
    C.row_view(lib)


@pytest.mark.parametrize("w", [1000, 4097])
def test_window_builder_matrices(lib, w):
    C.builder_products(lib, w, {})


def test_cache_invalidation(lib):
    C.cache_invalidation(lib)


def test_non_finite_input(lib):
    C.non_finite(lib)


@pytest.mark.parametrize("name,method", C.KRYLOV_RUNS)
def test_one_krylov_iteration(lib, name, method):
    C.krylov_iteration(lib, name, method, "1")
