"""GPU suite (-m gpu) for the Krylov loops of csrc/linalg.inc past their first iteration: k iterations of CG, BiCGStab
and GMRES (pfv_solve with rtol = 1e-300, maxit = k) against longdouble references of the same k iterations
(tests/_krylov_cases.py) -- k_cg_tail and k_bicg_tail with the sums that become beta, rho and the reported residual,
the p recurrence, k_dot2; gmres_multi_dot and gmres_multi_axpy over one, two and three groups of kGmresGroup basis
vectors and 1, 2, 3, 65 and 1024 blocks, the second Gram-Schmidt pass, the Givens and back-substitution kernels, the
restart boundary, m = min(m, maxit), the start from x0; the un-fused updates around precond_apply with a preconditioner
that is known exactly (block lower-triangular, every block a dense inverse).  A converged solve cannot stand in for
these checks: all three loops stay consistent with wrong scalars and only lose iterations, and GMRES recomputes the
true residual at every restart.  The huge matrix (2048 * 1024 + 2049 rows) makes the grid-stride loops of the tails
and of k_dot2 run a second trip, caps the GMRES blocks at 1024 and sends more than 4096 partial sums through
k_reduce_stage.

Not reached here, and why:
- AMG, near-null-space AMG and the flow-ordered sweep as M: inexact operators, no closed form to restate; they have
  suites of their own (test_gpu_amg.py, the near-null-space and sweep suites).  precond_apply is reached through the
  block preconditioner and Jacobi only.
- the sharded loop (pfv_solve_sharded: merged five-sum reduction, halo exchange, PFV_SHARD_CHECK_EVERY): needs the
  caller's hooks or RCCL; the distributed suites run it.
- the true-residual restart of BiCGStab (kTrueResidualRestarts): only after the recursive residual has converged, which
  rtol = 1e-300 never lets happen.
- check_every = 5 (GMRES) / 10 (CG, BiCGStab) for n >= 200 000: with maxit = k the only read of the residual is the one
  of the last iteration ("the last iteration is always read"); which earlier iterations are read changes nothing a
  non-converging run returns.
- `hcol[i] += ysol[i]`, the second Gram-Schmidt pass's share of the Hessenberg column: with the basis kept orthonormal
  by that very pass, its coefficients are the rounding error of the first pass, so leaving them out moves H by O(u)
  and x_k by less than the noise (on the emulation build: at most 0.18 of the allowance, against 0.12 with them).  The
  second pass's projection itself is not separable from rounding either at these condition numbers.
- the Givens estimate of GMRES as a reported number: on an unconverged return gmres_solve overwrites it with the true
  residual of the x it returns; that figure is what the rel_residual checks compare.  The estimate still decides the
  lucky-breakdown stop of the diagonal case."""
import pytest

import porepy_amd as pa
from tests import _krylov_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.fixture(autouse=True)
def windows_for_small_matrices(monkeypatch):
    monkeypatch.setenv("PFV_SPMV_WINDOW_MIN_NNZ", "0")
    for name in ("PFV_SPMV_WINDOW", "PFV_SPMV_U", "PFV_SPMV_L", "PFV_WIN_STRIDE", "PFV_WIN_ONEPASS", "PFV_DEBUG_WIN",
                 "PFV_SPMV_NT", "PFV_SPMV_BLOCKS", "PFV_AMG_FILTER_PERMIL", "PFV_TRUE_RESIDUAL"):
        monkeypatch.delenv(name, raising=False)


def ids(cases):
    return [K.label(c) for c in cases]


@pytest.mark.parametrize("window", ["1", "0"])
@pytest.mark.parametrize("case", K.CG_BICGSTAB + K.HUGE, ids=ids(K.CG_BICGSTAB + K.HUGE))
def test_cg_and_bicgstab_iterations(lib, case, window):
    """fused Jacobi (M == nullptr): MODE 2 / 3 of the windowed products (window 1), k_spmv_dot (window 0)"""
    K.check_iterations(lib, case, window)


@pytest.mark.parametrize("case", K.GMRES + [K.HUGE_GMRES], ids=ids(K.GMRES + [K.HUGE_GMRES]))
def test_gmres_iterations(lib, case):
    K.check_iterations(lib, case)


@pytest.mark.parametrize("case", K.BLOCK, ids=ids(K.BLOCK))
def test_iterations_with_a_known_preconditioner(lib, case):
    """M != nullptr: block Jacobi and block Gauss-Seidel with exact blocks, rows ascending and shuffled"""
    K.check_iterations(lib, case)


@pytest.mark.parametrize("method", ["cg", "bicgstab", "gmres"])
def test_zero_right_hand_side(lib, method):
    K.zero_rhs(lib, method)


@pytest.mark.parametrize("single_entry", [False, True], ids=["random_b", "one_entry"])
def test_gmres_lucky_breakdown_on_a_diagonal_matrix(lib, single_entry):
    K.diagonal_breakdown(lib, single_entry)
