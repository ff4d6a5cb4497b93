"""The host build of the guide pass (tests/cpp/guides_host.cpp: vk_raytrace_amd/csrc/pt_guides.h compiled by g++) and its Python side.  A library of
its own with its own g++ call -- the compile flags are host_harness.build's -- cached under tests/cpp/_build/.  It works on the scene handle a
host_harness.TracedScene (or Traced) holds, with the camera th_set_camera gave it.  A plain module: no test lives here."""
import ctypes as C
import glob
import os
import subprocess
import tempfile

import numpy as np

from vk_raytrace_amd import host_device as hd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BUILD_DIR = os.path.join(CPP, "_build")
OUT = os.path.join(BUILD_DIR, "libguideshost.so")
UNIT = os.path.join(CPP, "guides_host.cpp")
COMPILE = ["-std=c++17", "-O2", "-fopenmp", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-DSTACK_LDS=24", "-Wno-attributes",
           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "vk_raytrace_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
_lib = None


def _sources():
    """the unit, the harness headers it includes and every header of the product (the unit reaches most of them through pt_shade.h)"""
    return [UNIT, os.path.abspath(__file__)] + glob.glob(os.path.join(CPP, "th_*.h")) + glob.glob(os.path.join(ROOT, "vk_raytrace_amd", "csrc", "*.h")) + \
        glob.glob(os.path.join(ROOT, "include", "*.h"))


def build():
    """libguideshost.so, compiled if it is missing or older than a source it is made of; returns its path"""
    if os.path.exists(OUT) and all(os.path.getmtime(s) <= os.path.getmtime(OUT) for s in _sources()):
        return OUT
    os.makedirs(BUILD_DIR, exist_ok=True)
    fd, tmp = tempfile.mkstemp(suffix=".so", dir=BUILD_DIR)   # concurrent builders each write a file of their own; nobody loads a half-written one
    os.close(fd)
    try:
        subprocess.check_call(["g++"] + COMPILE + ["-shared", "-o", tmp, UNIT])
        os.replace(tmp, OUT)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return OUT


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        P = C.c_void_p
        L.gh_guides.restype, L.gh_guides.argtypes = C.c_uint32, [P, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_float, P, P, P]
        L.gh_rays.restype, L.gh_rays.argtypes = C.c_uint32, [P, C.c_int, C.c_int, P, P, P, P]
        _lib = L
    return _lib


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
