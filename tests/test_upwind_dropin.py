"""``pp.Upwind`` against ``porepy_amd.as_porepy_upwind()`` with the reference package itself importable (the same two
variants as tests/test_reference_dropin.py: emulation build on the CPU, HIP library on the GPU)."""
import pytest

from tests.test_reference_dropin import VARIANTS, run_script


@pytest.mark.parametrize("variant", VARIANTS)
def test_rebound_upwind_reproduces_the_reference(variant):
    out = run_script("_dropin_upwind_script.py", variant, 300)
    for name in ("cart2d", "cart2d_custom_flux_key", "cart2d_two_components", "tet3d_default_bc", "line1d"):
        o = out[name]
        assert o["is_subclass"] and o["matrices_identical"], (name, o)
        if "A_rel_err" in o:
            assert o["A_rel_err"] <= 1e-10 and o["rhs_rel_err"] <= 1e-10, (name, o)
        # the flux helper: a dot product per face, summed in another order than the reference's loop
        assert o["flux_helper_err"] <= 1e-15 and o["flux_helper_aperture_err"] <= 1e-15, (name, o)
