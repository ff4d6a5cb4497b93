"""The responsive history through the header-only C++ shim (include/pt_renderer.hpp temporalFast / readTemporalFast, tests/cpp/fast_shim_test.cpp): it
compiles against the C ABI, links with libptmi.so, and either runs one round whose checksums equal those of the same round through the Python route (GPU
box) or fails loudly with PT_ERR_NO_DEVICE."""
import numpy as np
import pytest

from tests import shim
from tests.shim import fnv


def test_cpp_shim_with_the_responsive_history_builds_and_fails_loudly_without_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "fast_shim_test"))   # (exit status 0)
    assert verdict in ("NO_DEVICE", "OK")


def python_route():
    """the round of fast_shim_test.cpp through HipRenderer: the same planes, images and camera, word for word"""
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
        r.temporal_fast(r.fast_params(2.0, 1.0, 2))
        r.set_denoise_guides(None, normal, depth)
        cam = Camera(eye=(0, 0, 5), center=(0, 0, 0), up=(0, 1, 0), fov=60.0)
        r.set_camera(capi.camera_lookat(cam, aspect))
        for k in range(4):
            img = shim.image(w, h, k)
            r.write_accum(img * np.float32(3.0) if k == 3 else img)
            out = r.temporal_accumulate(r.temporal_params(r.world_to_clip(cam, aspect), 0.05, 0.05, 8.0))
        _, length = r.read_temporal_history()
        fast, fast_length = r.read_temporal_fast()
        assert (length < 4).any() and (fast_length == 2).all()       # the brighter image was clamped in, and the lengths cut there
        return {"returned": fnv(out), "length": fnv(length), "fast": fnv(fast), "fastLength": fnv(fast_length), "shown": fnv(r.tonemap_history(None, hd.default_tonemapper()))}
    finally:
        r.destroy()


@pytest.mark.gpu
def test_cpp_shim_round_equals_the_python_route(tmp_path):
    verdict, got = shim.run(shim.build_shim(tmp_path, "fast_shim_test"))
    assert verdict == "OK"
    assert got == python_route()
