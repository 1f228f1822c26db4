"""GPU suite (-m gpu) for the SpMV family of the Krylov solves: every product of csrc/spmv_win.inc (k_win_build in both
layouts, k_spmv_win, its preloading twin k_spmv_win_pre) and of csrc/linalg.inc (k_spmv, k_spmv_dot) against the exact
int64 reference and the longdouble reference with its a-priori bound (tests/_spmv_cases.py), at the row lengths, block
tails and window sizes where the kernels change path; the fused reductions through one Krylov iteration.  A converged
solve cannot stand in for these checks: CG and BiCGStab stay consistent for any alpha or omega, so a wrong fused dot
only costs iterations.

Paths of these kernels that the exported entry points do not reach, and why they are absent here:
- `blist` launches of k_spmv_win / k_spmv_win_pre (shard_spmv with PFV_SHARD_OVERLAP): only with the native RCCL
  transport of a multi-GPU solve, where the halo exchange runs on the second stream.
- the windowed L is not switchable: it follows nnz / nrows alone, so L = 32 is reached by the matrices with more than
  160 entries per row only (PFV_SPMV_L acts on the plain k_spmv).
- k_spmv_dot<L, U, DOT> takes U from nnz / nrows alone (spmv_dot does not read PFV_SPMV_U): the one-iteration cases run
  it at (L, U) = (8, 3), (16, 3), (32, 6), (8, 2) [spd L8], (16, 3) [spd L16] and (8, 1) [big spd], DOT 1 and 2.
- k_spmv_win<L <= 16, U <= 5, double, MODE 0> runs only with PFV_SPMV_PRELOAD=0, which a process reads once: the
  child of test_windowed_kernels_without_preload.  Its MODE 2 / 3 instances at L <= 16, U <= 5 would need a second
  child with a solve; the L = 32 and U = 6 instances of the same template run here (ladder L32).
- k_spmv_win_pre MODE 1 and the f32 products (MODE 1 / 4 / 5, k_amg_spmv, k_win_derive) belong to the AMG cycle:
  tests/test_gpu_amg.py."""
import json
import os
import subprocess
import sys

import pytest

import porepy_amd as pa
from tests import _spmv_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.fixture(autouse=True)
def windows_for_small_matrices(monkeypatch):
    monkeypatch.setenv("PFV_SPMV_WINDOW_MIN_NNZ", "0")
    for name in ("PFV_SPMV_WINDOW", "PFV_SPMV_U", "PFV_SPMV_L", "PFV_WIN_STRIDE", "PFV_WIN_ONEPASS", "PFV_DEBUG_WIN",
                 "PFV_SPMV_NT", "PFV_SPMV_BLOCKS"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("lanes", [8, 16, 32])
def test_ladder_products(lib, lanes):
    C.ladder_products(lib, lanes)


@pytest.mark.parametrize("n", C.TAIL_SIZES)
def test_block_and_pass_tails(lib, n):
    C.tail_products(lib, n)


def test_row_view(lib):
    C.row_view(lib)


@pytest.mark.parametrize("w", C.BUILDER_W)
def test_window_builder(lib, w, capfd):
    """one pass for W <= 1024, two passes for 1025..4096, plain CSR for 4097"""
    C.builder_products(lib, w, {}, lambda: capfd.readouterr().err)


@pytest.mark.parametrize("env", [{"PFV_WIN_ONEPASS": 0}, {"PFV_WIN_STRIDE": 16}, {"PFV_SPMV_WINDOW": 0}],
                         ids=["onepass_off", "stride_16", "window_off"])
def test_window_builder_switches(lib, env, capfd):
    """W = 1000 in the compact two-pass layout (asked for, or because the stride is too small), and without windows"""
    C.builder_products(lib, 1000, env, lambda: capfd.readouterr().err)


def test_cache_invalidation(lib):
    C.cache_invalidation(lib)


def test_non_finite_input(lib):
    C.non_finite(lib)


@pytest.mark.parametrize("window", ["1", "0"])
@pytest.mark.parametrize("name,method", C.KRYLOV_RUNS)
def test_one_krylov_iteration(lib, name, method, window):
    """MODE 2 / 3 of the windowed kernels (window 1), k_spmv_dot<., ., 1 / 2> (window 0); the big matrix leaves more
    than kRedBlocks per-block partial sums either way"""
    C.krylov_iteration(lib, name, method, window)


def test_windowed_kernels_without_preload():
    """One child process with PFV_SPMV_PRELOAD=0 (the switch is a function-local static); never retried."""
    env = dict(os.environ, PFV_SPMV_PRELOAD="0", PFV_SPMV_WINDOW_MIN_NNZ="0")
    for name in ("PFV_SPMV_WINDOW", "PFV_SPMV_U", "PFV_SPMV_L"):
        env.pop(name, None)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_spmv_child_script.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, "child exited with status %d:\n%s" % (run.returncode, run.stderr[-4000:])
    report = json.loads(run.stdout.strip().splitlines()[-1])
    assert report["preload"] == "0"
    cases = report["cases"]
    assert sorted((c["L"], c["U"]) for c in cases) == [(lanes, u) for lanes in (8, 16, 32) for u in C.PRELOAD_OFF_U]
    bad = [c for c in cases if c["wrong_rows"]]
    assert not bad, "PFV_SPMV_PRELOAD=0, exact reference: " + "; ".join(
        "%s L=%d U=%d: first wrong row %d (%d entries): got %s, want %s; %d rows wrong" % (
            c["matrix"], c["L"], c["U"], c["first_wrong_row"], c["row_entries"], c["got"], c["want"], c["wrong_rows"])
        for c in bad)
