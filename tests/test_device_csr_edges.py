"""The device CSR algebra at its class edges on the host-emulation library: see tests/_device_csr_edge_cases.py.

On this build a work item is one lane, so the cooperative parts of the product (network, run heads, keep mask,
compaction) run as plain loops: what these cases pin here is the arithmetic, the class selection (``spgemm_path`` and
``spgemm_lds_bytes`` are computed as on the device) and the host-side code -- the upload cache, the operators, the
input checks of the C ABI.  tests/test_gpu_device_csr.py runs the same list on the gfx950 library."""
import pytest

from tests import _device_csr_edge_cases as E
from tests import _parity as P


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


@pytest.mark.parametrize("case, args", E.CASES + E.EMULATION_ONLY)
def test_device_csr_edge(lib, monkeypatch, case, args):
    case(lib, monkeypatch, E.Hooks(), *args)
