"""The host build of the denoiser (tests/cpp/denoise_host.cpp: vk_raytrace_amd/csrc/pt_denoise.h compiled by g++) and its Python side.  A library of
its own with its own g++ call -- the compile flags are host_harness.build's -- cached under tests/cpp/_build/.  A plain module: no test lives here."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from vk_raytrace_amd import host_device as hd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BUILD_DIR = os.path.join(CPP, "_build")
OUT = os.path.join(BUILD_DIR, "libdenoisehost.so")
SOURCES = [os.path.join(CPP, "denoise_host.cpp"), os.path.join(ROOT, "vk_raytrace_amd", "csrc", "pt_denoise.h"), os.path.join(ROOT, "include", "pt_fpmath.h"),
           os.path.join(ROOT, "include", "pt_types.h"), os.path.join(ROOT, "include", "pt_api.h")]
COMPILE = ["-std=c++17", "-O2", "-fopenmp", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-DSTACK_LDS=24", "-Wno-attributes",
           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "vk_raytrace_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
_lib = None


def build():
    """libdenoisehost.so, compiled if it is missing or older than a source it is made of; returns its path"""
    if os.path.exists(OUT) and all(os.path.getmtime(s) <= os.path.getmtime(OUT) for s in SOURCES + [os.path.abspath(__file__)]):
        return OUT
    os.makedirs(BUILD_DIR, exist_ok=True)
    fd, tmp = tempfile.mkstemp(suffix=".so", dir=BUILD_DIR)   # concurrent builders each write a file of their own; nobody loads a half-written one
    os.close(fd)
    try:
        subprocess.check_call(["g++"] + COMPILE + ["-shared", "-o", tmp, SOURCES[0]])
        os.replace(tmp, OUT)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return OUT


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.dh_denoise.restype, L.dh_denoise.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(hd.DenoiseParams), C.c_void_p, C.c_void_p]
        L.dh_constants.restype, L.dh_constants.argtypes = C.c_int, [C.POINTER(hd.DenoiseParams), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        _lib = L
    return _lib


def params(iterations, sigma_color, sigma_guide=(1.0, 1.0, 1.0), flags=0):
    return hd.DenoiseParams(iterations=iterations, sigmaColor=sigma_color, sigmaGuide=tuple(sigma_guide), flags=flags)


def denoise(colour, guides, p, per_iteration=False):
    """dh_denoise: colour (H, W, 4) float32, guides a sequence of three planes (None: unset).  Returns (status, out) or (status, out, per-iteration
    images of shape (iterations, H, W, 4)); the images are None when the status is not 0."""
    colour = np.ascontiguousarray(colour, np.float32)
    h, w = colour.shape[:2]
    planes = [None if g is None else np.ascontiguousarray(g, np.float32) for g in guides]
    assert all(g is None or g.shape == colour.shape for g in planes)
    ptrs = (C.c_void_p * 3)(*[None if g is None else g.ctypes.data for g in planes])
    out = np.empty_like(colour)
    its = np.empty((max(int(p.iterations), 0),) + colour.shape, np.float32) if per_iteration and 1 <= p.iterations <= 8 else None
    rc = lib().dh_denoise(colour.ctypes.data, ptrs, w, h, C.byref(p), out.ctypes.data, None if its is None else its.ctypes.data)
    if rc != 0:
        return (rc, None, None) if per_iteration else (rc, None)
    return (rc, out, its) if per_iteration else (rc, out)


def constants(p, planes_set):
    """(status, inv_c[8], inv_g[3], terms): the fp32 constants denoise_constants derives"""
    inv_c, inv_g, terms = np.zeros(8, np.float32), np.zeros(3, np.float32), C.c_uint32()
    rc = lib().dh_constants(C.byref(p), planes_set, inv_c.ctypes.data, inv_g.ctypes.data, C.byref(terms))
    return rc, inv_c, inv_g, terms.value
