"""Child process of test_gpu_spmv.py::test_windowed_kernels_without_preload.  PFV_SPMV_PRELOAD is read once per
process (a function-local static of launch_spmv_win_u), so the f64 windowed kernels k_spmv_win<L <= 16, U <= 5> that
k_spmv_win_pre normally replaces can only run in a process of their own, started with PFV_SPMV_PRELOAD=0.  Runs the
ladder matrices (exact reference, PFV_SPMV_U in {2, 5}) on the product library and prints ONE JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("PFV_SPMV_PRELOAD") == "0" and os.environ.get("PFV_SPMV_WINDOW_MIN_NNZ") == "0"
    import torch  # (its HIP runtime has to come up before the library opens the device: tests/conftest.py)

    torch.cuda.init()
    import porepy_amd as pa
    from tests import _spmv_cases as C

    print(json.dumps({"preload": os.environ["PFV_SPMV_PRELOAD"], "cases": C.preload_off_report(pa._lib.product_library())}))


if __name__ == "__main__":
    main()
