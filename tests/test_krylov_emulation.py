"""CPU suite for the Krylov loops past their first iteration on the host-emulation build (the portable two-stage
reductions, no fused tails, no windows) and the self-checks of the references the cases of tests/_krylov_cases.py are
judged by; tests/test_gpu_krylov.py runs the same cases on the HIP library."""
import numpy as np
import pytest

from tests import _krylov_cases as K
from tests import _parity as P


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


@pytest.fixture(autouse=True)
def plain_environment(monkeypatch):
    for name in ("PFV_SPMV_WINDOW", "PFV_SPMV_U", "PFV_SPMV_L", "PFV_AMG_FILTER_PERMIL", "PFV_TRUE_RESIDUAL"):
        monkeypatch.delenv(name, raising=False)


def ids(cases):
    return [K.label(c) for c in cases]


# ---- the references themselves ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.CG_BICGSTAB + K.GMRES + K.BLOCK, ids=ids(K.CG_BICGSTAB + K.GMRES + K.BLOCK))
def test_reference_noise(case):
    """every case is a pin: 0 < noise <= 1e-13 (asserted where the reference is made); the reference makes progress on
    its own terms; for GMRES the longdouble restatement of gmres_solve lands on the property form -- both are longdouble
    computations of one vector, so their distance is to the float64 noise as the unit roundoffs are, 2^-11, and 8 times
    that is asked for"""
    ref = K.reference(case)
    print("%s: noise %.3e, residual noise %.3e" % (K.label(case), ref.noise, ref.res_noise))
    assert ref.allowed == 8.0 * ref.noise and ref.res_allowed == 8.0 * ref.res_noise
    x_start = np.zeros(ref.A.shape[0]) if ref.x0 is None else ref.x0
    assert float(ref.res) < float(K.true_residual(ref.A, ref.b, x_start))
    if case.method == "gmres":
        gap = K.loop_gap(case)
        print("longdouble restatement of gmres_solve against the property form: %.3e" % gap)
        assert gap <= 8 * 2.0 ** -11 * ref.noise, (gap, ref.noise)


def test_gmres_property_form_minimises_the_residual():
    """the property form against brute force: no x_0 + M^-1 (a combination of the first k Krylov vectors) has a smaller
    residual -- a perturbation of the minimiser's coefficients along every basis direction only increases it"""
    case = K.Case("ladder L8", "gmres", 4, 50)
    ref = K.reference(case)
    ops = K.Ops(ref.A, K.LD, "forward")
    M = K.jacobi(ops)
    base = float(np.sqrt(np.sum((ref.b - ops.mv(ref.x)) ** 2)))
    v = ref.b.astype(K.LD)
    for _ in range(case.k):
        for sign in (-1, 1):
            x = ref.x + sign * 1e-6 * M(v) * (np.abs(ref.x).max() / np.abs(M(v)).max())
            assert float(np.sqrt(np.sum((ref.b - ops.mv(x)) ** 2))) > base
        v = ops.mv(M(v))


def test_block_reference_inverts_the_block_lower_triangle():
    """M M^-1 v = v for the block lower-triangular part taken densely, and the shuffled and the ascending storage of a
    matrix give the same operator"""
    for name in ("spd L8", "ladder L8"):
        outs = []
        for asc in (True, False):
            A, b = K.system(name, asc)
            ops = K.Ops(A, K.LD, "forward")
            z = K.block_lower(ops, True)(b.astype(K.LD))
            ptr = list(K.BLOCK_PTR) + [A.shape[0]]
            lower = np.array(A.toarray(), dtype=K.LD)
            for p0, p1 in zip(ptr[:-1], ptr[1:]):
                lower[p0:p1, p1:] = 0
            assert float(np.abs(lower @ z - b).max()) <= 1e-17
            outs.append(z)
        assert float(np.abs(outs[0] - outs[1]).max()) <= 1e-17


# ---- the cases on the emulation library --------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.CG_BICGSTAB + K.HUGE, ids=ids(K.CG_BICGSTAB + K.HUGE))
def test_cg_and_bicgstab_iterations(lib, case):
    K.check_iterations(lib, case)


@pytest.mark.parametrize("case", K.GMRES + [K.HUGE_GMRES], ids=ids(K.GMRES + [K.HUGE_GMRES]))
def test_gmres_iterations(lib, case):
    K.check_iterations(lib, case)


@pytest.mark.parametrize("case", K.BLOCK, ids=ids(K.BLOCK))
def test_iterations_with_a_known_preconditioner(lib, case):
    K.check_iterations(lib, case)


@pytest.mark.parametrize("method", ["cg", "bicgstab", "gmres"])
def test_zero_right_hand_side(lib, method):
    K.zero_rhs(lib, method)


@pytest.mark.parametrize("single_entry", [False, True], ids=["random_b", "one_entry"])
def test_gmres_lucky_breakdown_on_a_diagonal_matrix(lib, single_entry):
    K.diagonal_breakdown(lib, single_entry)
