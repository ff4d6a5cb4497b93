"""The demodulated history through the header-only C++ shim (include/pt_renderer.hpp temporalDemodulate, tests/cpp/albedo_shim_test.cpp): it compiles
against the C ABI, links with libptmi.so, and either runs one round whose checksums equal those of the same round through the Python route (GPU box) or
fails loudly with PT_ERR_NO_DEVICE."""
import numpy as np
import pytest

from tests import shim
from tests.shim import fnv


def test_cpp_shim_with_the_demodulated_history_builds_and_fails_loudly_without_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "albedo_shim_test"))   # (exit status 0)
    assert verdict in ("NO_DEVICE", "OK")


def albedo_plane(w, h):
    """albedo_plane of albedo_shim_test.cpp, word for word"""
    ys, xs = np.mgrid[0:h, 0:w]
    a = np.ones((h, w, 4), np.float32)
    a[..., :3] = (np.float32(0.25) + ((7 * xs + 3 * ys) % 13).astype(np.float32) * np.float32(0.0625))[..., None]
    return a


def python_route():
    """the round of albedo_shim_test.cpp through HipRenderer: the same planes, images and camera, word for word"""
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
        r.temporal_demodulate(True)
        r.track_moments(True)
        r.set_denoise_guides(albedo_plane(w, h), normal, depth)
        cam = Camera(eye=(0, 0, 5), center=(0, 0, 0), up=(0, 1, 0), fov=60.0)
        r.set_camera(capi.camera_lookat(cam, aspect))
        for k in range(3):
            r.write_accum(shim.image(w, h, k))
            r.temporal_accumulate(r.temporal_params(r.world_to_clip(cam, aspect), 0.05, 0.05, 8.0), read=False)
        sp, tm = r.svgf_params(3, 4.0, 1.0e-4, (1.0e15, 0.3, 0.5), 2.5), hd.default_tonemapper()
        dp = hd.DenoiseParams(iterations=2, sigmaColor=0.5, sigmaGuide=(1.0e15, 0.3, 0.5), flags=0)
        hist, length = r.read_temporal_history()
        filtered, var = r.svgf_history(sp)
        return {"history": fnv(hist), "length": fnv(length), "filtered": fnv(filtered), "variance": fnv(var), "shown": fnv(r.tonemap_svgf(sp, tm)),
                "denoised": fnv(r.denoise_history(dp)), "shownHistory": fnv(r.tonemap_history(None, tm))}
    finally:
        r.destroy()


@pytest.mark.gpu
def test_cpp_shim_round_equals_the_python_route(tmp_path):
    verdict, got = shim.run(shim.build_shim(tmp_path, "albedo_shim_test"))
    assert verdict == "OK"
    assert got == python_route()
