"""The path queries through the header-only C++ shim (include/pt_renderer.hpp tracePaths / tracePathsDevice, tests/cpp/paths_shim_test.cpp): it compiles
against the C ABI, links with libptmi.so, and either traces the paths of a few rays at a quad (GPU box) -- with the records the Python route returns for
the same scene, environment and rays -- or fails loudly with PT_ERR_NO_DEVICE."""
import ctypes as C

import numpy as np
import pytest

from tests import shim
from vk_raytrace_amd import capi, host_device as hd
from vk_raytrace_amd.renderer import HipRenderer

FLAGS = ("-D__HIP_PLATFORM_AMD__=1", "-I/opt/rocm/include")   # (the program calls hipMalloc itself)


class Quad:
    """the scene of tests/cpp/paths_shim_test.cpp, field for field, as HipRenderer.set_scene takes one"""

    def desc(self):
        pos = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
        nrm = np.tile(np.array([0, 0, 1], np.float32), (4, 1))
        tan = np.tile(np.array([1, 0, 0, 1], np.float32), (4, 1))
        uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
        v = capi.pack_vertices(pos, nrm, tan, uv, np.ones((4, 4), np.float32))
        idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
        pm = (hd.PrimMesh * 1)(hd.PrimMesh(0, 4, 0, 6, 0))
        nd = (hd.Node * 1)(hd.Node((C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16)), 0))
        m = hd.GltfShadeMaterial()
        m.pbrBaseColorFactor = (0.75, 0.5, 0.25, 1.0)
        for name in ("pbrBaseColorTexture", "pbrMetallicRoughnessTexture", "emissiveTexture", "normalTexture", "transmissionTexture", "clearcoatTexture", "clearcoatRoughnessTexture", "thicknessTexture"):
            setattr(m, name, -1)
        m.pbrRoughnessFactor, m.ior, m.doubleSided, m.attenuationDistance = 1.0, 1.5, 0, 3.4e38
        m.attenuationColor = (1.0, 1.0, 1.0)
        m.uvTransform = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
        mats = (hd.GltfShadeMaterial * 1)(m)
        d = hd.SceneDesc(v.ctypes.data, 4, idx.ctypes.data, 6, C.addressof(pm), 1, C.addressof(nd), 1, C.addressof(mats), 1, None, 0, None, 0)
        return d, (v, idx, pm, nd, mats)


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
    st = hd.RtxState(maxDepth=4, maxSamples=3, fireflyClampThreshold=100.0, hdrMultiplier=1.0, maxHeatmap=65000)
    rays = np.zeros(5, hd.ray_dtype)
    rays["origin"] = [[0.5, -0.5, 3], [-0.5, 0.5, 3], [3, 3, 3], [0.5, -0.5, -3], [0, 0, 3]]
    rays["direction"] = [[0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, 1], [0, 0, 0]]
    rays["tmax"], rays["seed"] = 10.0, [1, 2, 3, 4, 5]
    got = r.trace_path_records(st, rays)
    r.destroy()
    return got


def test_cpp_shim_with_path_queries_builds_and_fails_loudly_without_gpu(tmp_path):
    verdict, _ = shim.run(shim.build_shim(tmp_path, "paths_shim_test", FLAGS))   # (exit status 0)
    assert verdict in ("NO_DEVICE", "OK")


@pytest.mark.gpu
def test_cpp_shim_traces_the_python_routes_records(tmp_path):
    verdict, said = shim.run(shim.build_shim(tmp_path, "paths_shim_test", FLAGS))
    assert verdict == "OK"
    for key, accel in (("flat", capi.PT_ACCEL_FLAT), ("two", capi.PT_ACCEL_TWO_LEVEL)):
        got = python_route(accel)
        assert np.array_equal(got["status"], [capi.PT_RAY_HIT, capi.PT_RAY_HIT, 0, 0, capi.PT_RAY_INVALID])
        assert shim.fnv(got) == said[key], (key, got)
