"""The variance-guided filter through the header-only C++ shim (include/pt_renderer.hpp trackMoments / readTemporalMoments / svgfVariance /
svgfHistory / tonemapSvgf, tests/cpp/svgf_shim_test.cpp): it compiles against the C ABI, links with libptmi.so, and either runs one round whose
checksums equal those of the same round through the Python route (GPU box) or fails loudly with PT_ERR_NO_DEVICE."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_temporal_shim import fnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_svgf_shim(tmp_path):
    exe = str(tmp_path / "svgf_shim_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "svgf_shim_test.cpp"),
                           "-L", os.path.join(ROOT, "vk_raytrace_amd"), "-l:libptmi.so", "-Wl,-rpath," + os.path.join(ROOT, "vk_raytrace_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    return exe


def test_cpp_shim_with_the_svgf_stage_builds_and_fails_loudly_without_gpu(tmp_path):
    out = subprocess.run([build_svgf_shim(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("NO_DEVICE") or out.stdout.startswith("OK")


def python_route():
    """the round of svgf_shim_test.cpp through HipRenderer: the same planes, images and camera, word for word"""
    from vk_raytrace_amd import capi, host_device as hd
    from vk_raytrace_amd.renderer import HipRenderer
    from vk_raytrace_amd.scene import Camera
    w, h = 40, 24
    aspect = float(np.float32(w) / np.float32(h))
    ys, xs = np.mgrid[0:h, 0:w]
    normal = np.zeros((h, w, 4), np.float32)
    normal[...] = (0.5, 0.5, 1.0, 1.0)
    depth = np.zeros((h, w, 4), np.float32)
    depth[..., 0] = np.float32(4.0) + ((xs * 3 + ys * 5) % 16).astype(np.float32) * np.float32(0.125)
    r = HipRenderer()
    r.setup(0)
    try:
        r.create((w, h))
        r.track_moments(True)
        r.set_denoise_guides(None, normal, depth)
        cam = Camera(eye=(0, 0, 5), center=(0, 0, 0), up=(0, 1, 0), fov=60.0)
        r.set_camera(capi.camera_lookat(cam, aspect))
        i = np.arange(w * h * 4, dtype=np.uint64)
        for k in range(3):
            img = (((i * np.uint64(37 + 4 * k)) % np.uint64(101)).astype(np.float32) / np.float32(50.0)).reshape(h, w, 4)
            r.write_accum(img)
            r.temporal_accumulate(r.temporal_params(r.world_to_clip(cam, aspect), 0.05, 0.05, 8.0), read=False)
        sp, tm = r.svgf_params(3, 4.0, 1.0e-4, (1.0, 0.3, 0.5), 2.5), hd.default_tonemapper()
        filtered, var = r.svgf_history(sp)
        return {"moments": fnv(r.read_temporal_moments()), "v0": fnv(r.svgf_variance(sp)), "filtered": fnv(filtered), "variance": fnv(var), "shown": fnv(r.tonemap_svgf(sp, tm))}
    finally:
        r.destroy()


@pytest.mark.gpu
def test_cpp_shim_round_equals_the_python_route(tmp_path):
    out = subprocess.run([build_svgf_shim(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    got = dict(kv.split("=") for kv in out.stdout.split()[1:])
    assert got == python_route()
