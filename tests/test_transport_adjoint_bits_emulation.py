"""CPU suite: the four transport adjoints on the host-emulation build keep the bits of
tests/golden/transport_adjoint_bits/emulation.npz (tests/_transport_adjoint_bits_cases.py);
tests/test_gpu_transport_adjoint_bits.py does the same for the HIP library."""
from tests import _parity as P
from tests import _transport_adjoint_bits_cases as C


def test_transport_adjoints_keep_their_bits():
    C.check(P.emulation_library(), "emulation.npz")
