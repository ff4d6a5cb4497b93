"""The temporal stage through the header-only C++ shim (include/pt_renderer.hpp temporalAccumulate / readTemporalHistory / denoiseHistory /
tonemapHistory, tests/cpp/temporal_shim_test.cpp): it compiles against the C ABI, links with libptmi.so, and either runs one round whose checksums
equal those of the same round through the Python route (GPU box) or fails loudly with PT_ERR_NO_DEVICE."""
import numpy as np
import pytest

from tests import shim
from tests.shim import fnv


def test_cpp_shim_with_the_temporal_stage_builds_and_fails_loudly_without_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "temporal_shim_test"))   # (exit status 0)
    assert verdict in ("NO_DEVICE", "OK")


def python_route():
    """the round of temporal_shim_test.cpp through HipRenderer: the same planes, images and cameras, word for word"""
    from tests import denoise_host as dh
    from vk_raytrace_amd import capi, host_device as hd
    from vk_raytrace_amd.renderer import HipRenderer
    from vk_raytrace_amd.scene import Camera
    w, h = 40, 24
    aspect = float(np.float32(w) / np.float32(h))
    normal, depth = shim.planes(w, h)
    r = HipRenderer()
    r.setup(0)
    try:
        r.create((w, h))
        r.set_denoise_guides(None, normal, depth)
        for k in range(2):
            x = float(np.float32(0.05) * np.float32(k))
            cam = Camera(eye=(x, 0, 5), center=(x, 0, 0), up=(0, 1, 0), fov=60.0)
            r.set_camera(capi.camera_lookat(cam, aspect))
            r.write_accum(shim.image(w, h, k))
            out = r.temporal_accumulate(r.temporal_params(r.world_to_clip(cam, aspect), 0.05, 0.05, 8.0))
        hc, hn = r.read_temporal_history()
        assert np.array_equal(hc.view(np.uint32), out.view(np.uint32))
        dp, tm = dh.params(2, 1.0, (1.0, 0.3, 0.5)), hd.default_tonemapper()
        return {"colour": fnv(out), "length": fnv(hn), "denoised": fnv(r.denoise_history(dp)), "shown": fnv(r.tonemap_history(None, tm)), "filtered": fnv(r.tonemap_history(dp, tm))}
    finally:
        r.destroy()


@pytest.mark.gpu
def test_cpp_shim_round_equals_the_python_route(tmp_path):
    verdict, got = shim.run(shim.build_shim(tmp_path, "temporal_shim_test"))
    assert verdict == "OK"
    assert got == python_route()
