"""The host build of the denoiser (tests/cpp/denoise_host.cpp: vk_raytrace_amd/csrc/pt_denoise.h compiled by g++) and its Python side.  The library is
one of host_harness.build_library's, cached under tests/cpp/_build/; it needs no libptmi.so.  A plain module: no test lives here."""
import ctypes as C

import numpy as np

from tests import host_harness as hh
from vk_raytrace_amd import host_device as hd

SIGNATURES = [
    ("dh_denoise", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(hd.DenoiseParams), C.c_void_p, C.c_void_p]),
    ("dh_constants", C.c_int, [C.POINTER(hd.DenoiseParams), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
]
_host = hh.StageLibrary("libdenoisehost", "denoise_host.cpp", SIGNATURES)
build, compile_to, bind, lib = _host.build, _host.compile_to, _host.bind, _host.lib


def params(iterations, sigma_color, sigma_guide=(1.0, 1.0, 1.0), flags=0):
    return hd.DenoiseParams(iterations=iterations, sigmaColor=sigma_color, sigmaGuide=tuple(sigma_guide), flags=flags)


def denoise(colour, guides, p, per_iteration=False):
    """dh_denoise: colour (H, W, 4) float32, guides a sequence of three planes (None: unset).  Returns (status, out) or (status, out, per-iteration
    images of shape (iterations, H, W, 4)); the images are None when the status is not 0."""
    colour = np.ascontiguousarray(colour, np.float32)
    h, w = colour.shape[:2]
    planes, ptrs = hh.planes_arg(guides, h, w)
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
