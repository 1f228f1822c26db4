"""GPU suite (-m gpu) for the near-null-space AMG (PFV_PRECOND_AMG_NNS): the cases of test_amg_nns_emulation.py on the
gfx950 HIP library, plus the larger configs[3]-family size."""
import pytest

import porepy_amd as pa
from tests import _amg_nns_cases as C
from tests import _amg_nns_cycle_cases as Y
from tests import _parity as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


def test_rigid_body_modes_are_a_null_space_2d(lib):
    C.modes_are_null_space(lib, C.grid_2d(8))


def test_rigid_body_modes_are_a_null_space_3d(lib):
    C.modes_are_null_space(lib, C.grid_3d(5))


def test_hierarchy_identities_mpsa(lib):
    C.mpsa_hierarchy(lib, 12)


def test_hierarchy_identities_user_system_with_singleton(lib):
    C.user_system_hierarchy(lib)


def test_device_modes_follow_the_renumbering(lib):
    C.reordering(lib, 12)


def test_split_path(lib):
    C.split_path(lib, 6)


def test_uniaxial_exact_3d(lib):
    P.mpsa_uniaxial_exact(lib, C.grid_3d(4, perturb=False), tol=1e-9, precond="amg_rbm")


def test_uniaxial_exact_2d(lib):
    P.mpsa_uniaxial_exact(lib, C.grid_2d(8), tol=1e-9, precond="amg_rbm")


def test_clamped_heterogeneous_against_direct(lib):
    C.clamped_against_direct(lib, 6)


@pytest.mark.parametrize("n", [16, 24])
def test_fewer_iterations_than_plain_amg(lib, n):
    C.fewer_iterations(lib, n)


def test_deterministic(lib):
    C.deterministic(lib, 10)


def test_plain_amg_untouched(lib):
    C.nothing_else_moved(lib, 10)


def test_sharded_unsupported(lib):
    C.sharded_unsupported(lib)


def test_bad_arguments(lib):
    C.bad_arguments(lib)


# the cycle against the independent reference (tests/_amg_nns_cycle_cases.py)

@pytest.mark.parametrize("name", list(Y.USER_CASES))
def test_cycle_against_reference(lib, name):
    Y.user_case(lib, name)


@pytest.mark.parametrize("name", list(Y.MPSA_CASES))
def test_cycle_against_reference_mpsa(lib, name):
    Y.mpsa_case(lib, name)


def test_too_wide_coarse_row_is_refused(lib):
    Y.too_wide_is_refused(lib)


def test_passes_stop_at_the_built_in_target(lib):
    Y.passes_stop_at_the_constant(lib)


def test_rigid_body_modes_far_from_the_origin(lib):
    Y.far_from_the_origin(lib)


def test_apply_is_read_only(lib):
    Y.apply_is_read_only(lib)
