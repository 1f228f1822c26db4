"""CPU suite: the flow-ordered forward transport steps on the host-emulation build keep the bits of
tests/golden/transport_forward_bits/emulation.npz (tests/_transport_forward_bits_cases.py);
tests/test_gpu_transport_forward_bits.py does the same for the HIP library."""
from tests import _parity as P
from tests import _transport_forward_bits_cases as C


def test_forward_transport_steps_keep_their_bits():
    C.check(P.emulation_library(), "emulation.npz")
