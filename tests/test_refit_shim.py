"""The deforming meshes through the header-only C++ shim (include/pt_renderer.hpp updateVertices / refitAccel, tests/cpp/refit_shim_test.cpp): it compiles
against the C ABI, links with libptmi.so, and either renders two frames of a quad after its vertices moved and the structure was refitted (GPU box) -- the
images the Python route renders on the same scene, environment and camera -- or fails loudly with PT_ERR_NO_DEVICE."""
import ctypes as C

import numpy as np
import pytest

from tests import shim
from tests.test_paths_shim import Quad
from vk_raytrace_amd import capi, host_device as hd
from vk_raytrace_amd.renderer import HipRenderer

MOVED = np.array([[-0.75, -0.5, 0.25], [0.5, -0.75, -0.125], [0.75, 0.5, 0.5], [-0.5, 0.75, 0.0]], np.float32)


def python_route(accel):
    r = HipRenderer(); r.setup(0)
    r.set_accel_mode(accel)
    quad = Quad()
    r.set_scene(quad)
    i = np.arange(32)
    env = np.stack([(i % 5 + 1) * 0.25, (i % 3 + 1) * 0.25, (i % 7 + 1) * 0.125, np.ones(32)], 1).astype(np.float32).reshape(4, 8, 4)
    r.set_env(env)
    cam = hd.SceneCamera()
    e, c, u = (np.asarray(x, np.float32) for x in ((0, 0, 3), (0, 0, 0), (0, 1, 0)))
    assert capi.lib().pt_camera_lookat(e.ctypes.data, c.ctypes.data, u.ctypes.data, 60.0, 1.0, C.byref(cam)) == capi.PT_OK
    r.set_camera(cam)
    r.create((32, 32))
    v = capi.pack_vertices(MOVED, np.tile(np.float32([0, 0, 1]), (4, 1)), np.tile(np.float32([1, 0, 0, 1]), (4, 1)), np.float32([[0, 0], [1, 0], [1, 1], [0, 1]]), np.ones((4, 4), np.float32))
    r.update_vertices(0, v)
    info = r.refit_accel()
    assert info.slotsWritten == 2 and info.nodesWritten == 1 and info.costAfter < info.costBefore
    st = hd.RtxState(maxDepth=3, maxSamples=1, fireflyClampThreshold=100.0, hdrMultiplier=1.0, maxHeatmap=65000)
    for f in range(2):
        st.frame = f
        r.setPushContants(st)
        r.run()
    img = r.read_accum()
    r.destroy()
    return img


def test_cpp_shim_with_refit_builds_and_fails_loudly_without_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "refit_shim_test"))   # (exit status 0)
    assert verdict in ("NO_DEVICE", "OK")


@pytest.mark.gpu
def test_cpp_shim_renders_the_python_routes_frames_after_a_refit(tmp_path):
    verdict, said = shim.run(shim.build_shim(tmp_path, "refit_shim_test"))
    assert verdict == "OK"
    for key, accel in (("flat", capi.PT_ACCEL_FLAT), ("two", capi.PT_ACCEL_TWO_LEVEL)):
        img = python_route(accel)
        assert img[..., :3].max() > 0 and shim.fnv(img) == said[key], key
    assert said["flat"] == said["two"]
