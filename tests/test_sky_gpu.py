"""The device's sun_and_sky (csrc/pt_sky.h through pt_debug_shading_probe case SUN_AND_SKY, one row per lane) on every stored row of tests/golden/sky_kat.npz:
bit-identical to the host build of the same header on ALL rows, the rays at the sun and the ill-conditioned rows included, and within the class bounds of
tests/golden/sky_kat_tol.json (4 x the compiled reference's recorded maximum per class) on the kept ones.  Reads the committed fixture only; one launch."""
import ctypes as C

import numpy as np
import pytest

from tests import sky_kat_io as io


@pytest.mark.gpu
def test_device_sun_and_sky_is_the_host_build_and_meets_the_model():
    from tests import host_harness
    from vk_raytrace_amd import capi
    kat, tol = io.load(), io.tolerances()
    L = capi.lib()
    ctx = C.c_void_p()
    assert L.pt_create(0, C.byref(ctx)) == 0
    try:
        got = io.through_probe(L.pt_debug_shading_probe, ctx)(kat["rows"])
    finally:
        L.pt_destroy(ctx)
    host = io.through_probe(host_harness.lib().th_shading_probe)(kat["rows"])
    bad = io.same_bits(got, host)
    rows = np.where((got.view(np.uint32) != host.view(np.uint32)).any(1))[0]
    assert bad == 0, f"device and host build differ in {bad} values, first at row {rows[:1]} ({kat['setting_names'][kat['row_setting'][rows[:1]]]})"
    io.check(kat, tol, got, "device")
