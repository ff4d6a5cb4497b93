"""The gather queries through the header-only C++ shim (include/pt_renderer.hpp gatherIrradiance / gatherProbes / gatherDevice,
tests/cpp/gather_shim_test.cpp): it compiles against the C ABI, links with libptmi.so, and either gathers at a few points at a quad (GPU box) -- with the
records the Python route returns for the same scene, environment and points -- or fails loudly with PT_ERR_NO_DEVICE."""
import ctypes as C

import numpy as np
import pytest

from tests import shim
from tests.test_paths_shim import FLAGS, Quad
from vk_raytrace_amd import capi, host_device as hd
from vk_raytrace_amd.renderer import HipRenderer


def python_route(accel):
    r = HipRenderer(); r.setup(0)
    r.set_accel_mode(accel)
    r.set_scene(Quad())
    i = np.arange(32)
    env = np.stack([(i % 5 + 1) * 0.25, (i % 3 + 1) * 0.25, (i % 7 + 1) * 0.125, np.ones(32)], 1).astype(np.float32).reshape(4, 8, 4)
    r.set_env(env)
    cam = hd.SceneCamera()
    e, c, u = (np.asarray(x, np.float32) for x in ((0, 0, 3), (0, 0, 0), (0, 1, 0)))
    assert capi.lib().pt_camera_lookat(e.ctypes.data, c.ctypes.data, u.ctypes.data, 60.0, 1.0, C.byref(cam)) == capi.PT_OK
    r.set_camera(cam)
    st = hd.RtxState(maxDepth=4, maxSamples=8, fireflyClampThreshold=100.0, hdrMultiplier=1.0, maxHeatmap=65000)
    pos = [[0, 0, 0.01], [0.5, 0.5, 0], [3, 3, 1], [0, 0, -1], [0, 0, 1]]
    nrm = [[0, 0, -2], [0, 0, 1], [-1, -1, -0.5], [0, 0, 1], [0, 0, 0]]
    got = r.gather_irradiance(st, pos, nrm, [1, 2, 3, 4, 5]), r.gather_probes(st, pos, [1, 2, 3, 4, 5])
    r.destroy()
    return got


def test_cpp_shim_with_gather_queries_builds_and_fails_loudly_without_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "gather_shim_test", FLAGS))   # (exit status 0)
    assert verdict in ("NO_DEVICE", "OK")


@pytest.mark.gpu
def test_cpp_shim_gathers_the_python_routes_records(tmp_path):
    verdict, said = shim.run(shim.build_shim(tmp_path, "gather_shim_test", FLAGS))
    assert verdict == "OK"
    for key, accel in (("flat", capi.PT_ACCEL_FLAT), ("two", capi.PT_ACCEL_TWO_LEVEL)):
        irr, probes = python_route(accel)
        assert np.array_equal(irr["status"], [0, 0, 0, 0, capi.PT_RAY_INVALID]) and (probes["status"] == 0).all()
        assert shim.fnv(irr) == said[key] and shim.fnv(probes) == said[key + "_probes"], (key, irr, probes)
