"""GPU suite (-m gpu): the device CSR algebra at its lane-group and class edges.

The product of two device matrices sorts the products feeding a row in LDS with 16, 32 or 64 lanes: a bitonic network
over P2 / 2 lanes, run heads found by neighbouring lanes, a keep mask built with atomicOr, a compaction by popcount over
the mask words, up to four rows of different length in one wavefront.  None of that is in the host-emulation build,
where a work item is one lane.  tests/_device_csr_edge_cases.py puts a row on either side of every edge (lane-group
width, power of two, mask word, the 48 KiB opt-in of the LDS, the switch to the global sorts) and compares with scipy
bit for bit; every case asserts from ``stats()`` the path and the LDS bytes of the launch it was written for.  The two
malformed ``indptr`` inputs of the C ABI are left to the emulation suite (tests/test_device_csr_edges.py): see
``abi_indptr_is_checked_on_the_host``."""
import pytest

import porepy_amd as pa
from tests import _device_csr_edge_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()  # raises if the HIP build is missing


@pytest.fixture(scope="module")
def hooks():
    import torch

    def to_device(a):
        t = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        return t.data_ptr(), t

    return E.Hooks(to_device, lambda t: t.cpu().numpy())


@pytest.mark.parametrize("case, args", E.CASES)
def test_device_csr_edge(lib, hooks, monkeypatch, case, args):
    case(lib, monkeypatch, hooks, *args)
