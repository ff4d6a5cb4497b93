"""The host build of the guide pass (tests/cpp/guides_host.cpp: vk_raytrace_amd/csrc/pt_guides.h compiled by g++) and its Python side.  The library is
one of host_harness.build_library's, cached under tests/cpp/_build/.  It works on the scene handle a host_harness.TracedScene (or Traced) holds, with
the camera th_set_camera gave it.  A plain module: no test lives here."""
import ctypes as C

import numpy as np

from tests import host_harness as hh
from vk_raytrace_amd import host_device as hd

_P = C.c_void_p
SIGNATURES = [
    ("gh_guides", C.c_uint32, [_P, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_float, _P, _P, _P]),
    ("gh_rays", C.c_uint32, [_P, C.c_int, C.c_int, _P, _P, _P, _P]),
]
_host = hh.StageLibrary("libguideshost", "guides_host.cpp", SIGNATURES)
build, compile_to, bind, lib = _host.build, _host.compile_to, _host.bind, _host.lib


def set_camera(traced, camera: hd.SceneCamera, sunsky=None):
    """th_set_camera on a host_harness.Traced / TracedScene"""
    ss = sunsky if sunsky is not None else hd.default_sun_and_sky()
    traced.L.th_set_camera(traced.h, C.byref(camera), C.byref(ss))


def guides(traced, two, width, height, planes=7, miss_depth=1.0e30, into=None):
    """gh_guides: the three planes, (H, W, 4) float32 each, of the scene `traced` holds for the camera set_camera gave it.  A plane outside `planes`
    is not written: it keeps what `into` (a sequence of three arrays) holds, or comes back as None."""
    out = [None] * 3
    for j in range(3):
        if into is not None and into[j] is not None:
            out[j] = into[j]
            assert out[j].dtype == np.float32 and out[j].shape == (height, width, 4) and out[j].flags.c_contiguous
        elif planes & (1 << j):
            out[j] = np.zeros((height, width, 4), np.float32)
    over = lib().gh_guides(traced.h, int(two), width, height, planes, miss_depth, *[None if p is None else p.ctypes.data for p in out])
    assert over == 0, "traversal stack overflow"
    return tuple(out)


def rays(traced, width, height):
    """gh_rays: (org (n, 3), dir (n, 3), seed_after_camera (n,), seed_after_walk (n,)) per pixel in row-major order"""
    n = width * height
    org, dirs = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    s0, s1 = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    over = lib().gh_rays(traced.h, width, height, org.ctypes.data, dirs.ctypes.data, s0.ctypes.data, s1.ctypes.data)
    assert over == 0, "traversal stack overflow"
    return org, dirs, s0, s1
