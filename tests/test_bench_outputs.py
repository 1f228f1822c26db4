"""CPU suite: what ``bench.py --dump-outputs`` writes, on a small grid of the timed workload family, with the host
emulation of the kernel sources behind the same calls the timed step makes."""
import os

import numpy as np
import pytest

import bench
import porepy_amd as pa
from tests import _parity as P


@pytest.fixture(scope="module")
def solved():
    lp, Kv, flags, bv, src, eta = bench.make_slab_problem(6, 0, 1, strong=True, blocks=(1, 1, 1))
    ctx = pa.Context(0, P.emulation_library())
    ctx.set_grid(lp.raw)
    ctx.set_params(Kv, flags, None, eta)
    ctx.discretize(rebuild_topology=True)
    ctx.assemble(bv, None, src)
    x, info = ctx.solve("bicgstab", rtol=1e-13, maxit=2000, raise_on_fail=False, precond="jacobi")
    assert info["converged"]
    yield lp, ctx, np.array(x)
    ctx.close()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_the_step_result_in_global_cell_order(solved, tmp_path):
    lp, ctx, x = solved
    bench.dump_outputs(str(tmp_path), pa, ctx, x, lp, None, 0)
    out = _load(tmp_path)
    assert sorted(out) == ["pressure", "rhs", "system_matrix_times_probe"]
    order = np.argsort(lp.cell_gid)
    A = ctx.matrix(pa._lib.MAT_SYSTEM)
    probe = bench._hash_normal(np.asarray(lp.cell_gid, dtype=np.int64), bench.DUMP_PROBE_SALT)
    for k in out:
        assert out[k].dtype == np.float64 and out[k].shape == (lp.n_own,)
    assert np.array_equal(out["pressure"], x[order])
    assert np.array_equal(out["rhs"], np.asarray(ctx.rhs())[order])
    assert np.allclose(out["system_matrix_times_probe"], (A @ probe)[order], rtol=1e-13, atol=1e-13 * np.abs(A).max())
    # the same call again writes the same arrays
    again = tmp_path / "again"
    bench.dump_outputs(str(again), pa, ctx, x, lp, None, 0)
    assert all(np.array_equal(v, _load(again)[k]) for k, v in out.items())


def test_dump_above_the_size_limit_is_a_fixed_sample(solved, tmp_path, monkeypatch):
    lp, ctx, x = solved
    full = tmp_path / "full"
    bench.dump_outputs(str(full), pa, ctx, x, lp, None, 0)
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 8 * 4 * 300)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), pa, ctx, x, lp, None, 0)
    bench.dump_outputs(str(b), pa, ctx, x, lp, None, 0)
    sa, sb, ref = _load(a), _load(b), _load(full)
    assert sorted(sa) == ["cell_ids", "pressure", "rhs", "system_matrix_times_probe"]
    assert sum(os.path.getsize(a / f) - 128 for f in os.listdir(a)) <= 8 * 4 * 300  # (npy headers aside)
    ids = sa["cell_ids"].astype(np.int64)
    assert ids.size == 300 and np.all(np.diff(ids) > 0)
    for k in ("pressure", "rhs", "system_matrix_times_probe"):
        assert np.array_equal(sa[k], ref[k][ids])
        assert np.array_equal(sa[k], sb[k])


def test_permeability_factors_drawn_in_threads_equal_the_serial_draw():
    gid = np.arange(20000, dtype=np.int64)[::-1].copy()
    got = bench.permeability_factors(gid, 11)
    assert len(got) == 10
    for i, f in enumerate(got, start=1):
        assert np.array_equal(f, np.exp(0.5 * bench._hash_normal(gid, 1000 + 2 * i)))
