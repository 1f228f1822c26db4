"""GPU suite (-m gpu): the four transport adjoints on the gfx950 HIP library keep the bits of
tests/golden/transport_adjoint_bits/gfx950.npz (tests/_transport_adjoint_bits_cases.py)."""
import pytest

import porepy_amd as pa
from tests import _transport_adjoint_bits_cases as C

pytestmark = pytest.mark.gpu


def test_transport_adjoints_keep_their_bits():
    C.check(pa._lib.product_library(), "gfx950.npz")
