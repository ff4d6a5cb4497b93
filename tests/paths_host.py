"""The host build of the path query: vk_raytrace_amd/csrc/pt_paths.h (path_query<TWO>, what pt_trace_paths' kernel runs per lane)
compiled by g++ from tests/cpp/paths_host.cpp into a library of its own next to the units of the host harness (tests/host_harness.py), and its Python
side: the binding, a scene with environment and camera installed, and the calls the host tests (tests/test_paths_host.py) and the device tests that take
this build as their reference (tests/test_paths_gpu.py) share.  A plain module: no test lives here."""
import ctypes as C

import numpy as np

from tests import host_harness
from vk_raytrace_amd import host_device as hd

_P, _I, _U = C.c_void_p, C.c_int, C.c_uint32
NAME = "libpathshost"
# tests/cpp/paths_host.cpp: (name, restype, argtypes)
SIGNATURES = [
    ("ph_paths", _U, [_P, _I, C.POINTER(hd.RtxState), _I, C.c_uint64, _P, _P]),          # (scene, two, state, variant, n, rays, results) -> overflows
    ("ph_camera_rays", None, [_P, C.POINTER(hd.RtxState), _I, _P]),                       # (scene, state, variant, rays out[size])
    ("ph_path_segments", _U, [_P, _I, C.POINTER(hd.RtxState), _I, _P, _P, _U]),           # (scene, two, state, variant, ray, segments out[cap], cap) -> segments
]
LCG_MUL, LCG_ADD = 747796405, 2891336453   # rng_next's state step (pt_math.h; shaders/random.glsl)
_lib = None


def build():
    """tests/cpp/_build/libpathshost.so: the harness's units and paths_host.cpp (the Scene of th_scene.h is one struct in both libraries)"""
    return host_harness.build_library(NAME, host_harness.UNITS + ["paths_host.cpp"], needs_libptmi=True)


def lib():
    global _lib
    if _lib is None:
        _lib = host_harness.bind(build(), host_harness.SIGNATURES + SIGNATURES)
    return _lib


def advance(seed, draws):
    """the RNG state `draws` draws later"""
    s = np.asarray(seed, np.uint64)
    for _ in range(draws):
        s = (s * np.uint64(LCG_MUL) + np.uint64(LCG_ADD)) & np.uint64(0xFFFFFFFF)
    return s.astype(np.uint32)


class PathScene:
    """cfg (tests.common.Config) on the harness with its environment, camera and sun & sky installed: what pt_trace_paths needs of the scene side.
    `tr` is a host_harness.TracedScene; its handle serves both libraries."""

    def __init__(self, cfg):
        self.cfg, self.L = cfg, lib()
        self.tr = host_harness.TracedScene(cfg.scene)
        integral = C.c_float()
        assert self.L.th_set_env(self.tr.h, cfg.env.ctypes.data, cfg.env.shape[1], cfg.env.shape[0], C.byref(integral)) == 0
        self.L.th_set_camera(self.tr.h, C.byref(cfg.camera), C.byref(cfg.sunsky))
        self.integral = integral.value

    def state(self, **fields):
        st = self.cfg.state(self.integral)
        for k, v in fields.items():
            setattr(st, k, v)
        return st

    def camera_rays(self, st=None):
        """the camera rays of frame st.frame (default 0), sample 0, row-major, with the seed after the camera's draws: hd.ray_dtype records"""
        st = st or self.state()
        rays = np.zeros(st.size[0] * st.size[1], hd.ray_dtype)
        self.L.ph_camera_rays(self.tr.h, C.byref(st), self.cfg.variant, rays.ctypes.data)
        return rays

    def paths(self, two, st, rays, variant=None, overflow=False):
        """path_query on the host: (n,) hd.pathresult_dtype records.  overflow: also return the traversal-stack overflows"""
        rays = np.ascontiguousarray(rays, hd.ray_dtype)
        out = np.zeros(len(rays), hd.pathresult_dtype)
        over = self.L.ph_paths(self.tr.h, int(two), C.byref(st), self.cfg.variant if variant is None else int(variant), len(rays), rays.ctypes.data, out.ctypes.data)
        if overflow:
            return out, over
        assert over == 0, "traversal stack overflow"
        return out

    def segments(self, two, st, ray, variant=None, cap=4096):
        """every ray the paths of one ray traced, in order, as hd.ray_dtype records: tmax is the ray's bound, seed its kind (PT_RAYS_CLOSEST / OCCLUDED)"""
        one = np.ascontiguousarray(ray, hd.ray_dtype).reshape(1)
        out = np.zeros(cap, hd.ray_dtype)
        n = self.L.ph_path_segments(self.tr.h, int(two), C.byref(st), self.cfg.variant if variant is None else int(variant), one.ctypes.data, out.ctypes.data, cap)
        assert n <= cap
        return out[:n]

    def close(self):
        self.tr.close()
