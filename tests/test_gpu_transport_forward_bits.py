"""GPU suite (-m gpu): the flow-ordered forward transport steps on the gfx950 HIP library keep the bits of
tests/golden/transport_forward_bits/gfx950.npz (tests/_transport_forward_bits_cases.py)."""
import pytest

import porepy_amd as pa
from tests import _transport_forward_bits_cases as C

pytestmark = pytest.mark.gpu


def test_forward_transport_steps_keep_their_bits():
    C.check(pa._lib.product_library(), "gfx950.npz")
