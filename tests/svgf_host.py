"""The host build of the variance-guided filter (tests/cpp/svgf_host.cpp: vk_raytrace_amd/csrc/pt_svgf.h compiled by g++) and its Python side.  The
library is one of host_harness.build_library's, cached under tests/cpp/_build/; it needs no libptmi.so.  A plain module: no test lives here."""
import ctypes as C

import numpy as np

from tests import history_host as hs, host_harness as hh
from vk_raytrace_amd import host_device as hd

CSRC = hh.CSRC
_P = C.c_void_p
_G = C.POINTER(_P)
SIGNATURES = [
    ("sh_temporal_m", C.c_int, hs.STEP),
    hs.LAYOUT,
    ("sh_variance", C.c_int, [_P, _P, _P, _G, C.c_int, C.c_int, C.POINTER(hd.SvgfParams), _P]),
    ("sh_iteration", C.c_int, [_P, _P, _G, C.c_int, C.c_int, C.POINTER(hd.SvgfParams), C.c_int, _P, _P]),
    ("sh_constants", C.c_int, [C.POINTER(hd.SvgfParams), C.c_uint, C.c_char_p, C.c_int]),
]
_host = hh.StageLibrary("libsvgfhost", "svgf_host.cpp", SIGNATURES)
build, compile_to, bind, lib = _host.build, _host.compile_to, _host.bind, _host.lib


def params(iterations, sigma_lum=4.0, lum_floor=1e-4, sigma_guide=(1.0, 1.0, 1.0), min_temporal=3.5, flags=0):
    p = hd.SvgfParams(iterations=iterations, flags=flags)
    words = np.array([sigma_lum, lum_floor, *sigma_guide, min_temporal], np.float32)          # bit patterns as given (NaN included)
    C.memmove(C.addressof(p) + 4, words.ctypes.data, 24)
    return p


def History(colour, guide, length, moments, world_to_clip, eye):
    """history_host.History with the moments image, in this module's argument order"""
    return hs.History(colour, guide, length, world_to_clip, eye, moments)


def temporal_m(colour, normal, depth, view_inverse, proj_inverse, p, hist=None, L=None):
    """sh_temporal_m: one call with tracking on.  Returns (status, History or None)"""
    return hs.run((L or lib()).sh_temporal_m, colour, normal, depth, view_inverse, proj_inverse, p, hist, moments=True)[:2]


def variance(hist_colour, hist_length, hist_moments, guides, p, L=None):
    """sh_variance: (status, V0 (H, W) or None)"""
    hc, hn, hm = (np.ascontiguousarray(a, np.float32) for a in (hist_colour, hist_length, hist_moments))
    h, w = hn.shape
    assert hc.shape == (h, w, 4) and hm.shape == (h, w, 2)
    keep, ptrs = hh.planes_arg(guides, h, w)
    out = np.empty((h, w), np.float32)
    rc = (L or lib()).sh_variance(hc.ctypes.data, hn.ctypes.data, hm.ctypes.data, ptrs, w, h, C.byref(p), out.ctypes.data)
    return rc, (out if rc == 0 else None)


def iteration(colour, var, guides, p, i, L=None):
    """sh_iteration: (status, colour (H, W, 4), variance (H, W)) of iteration i alone"""
    c, v = np.ascontiguousarray(colour, np.float32), np.ascontiguousarray(var, np.float32)
    h, w = v.shape
    assert c.shape == (h, w, 4)
    keep, ptrs = hh.planes_arg(guides, h, w)
    oc, ov = np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32)
    rc = (L or lib()).sh_iteration(c.ctypes.data, v.ctypes.data, ptrs, w, h, C.byref(p), i, oc.ctypes.data, ov.ctypes.data)
    return (rc, oc, ov) if rc == 0 else (rc, None, None)


def filter_history(hist, guides, p, L=None):
    """pt_svgf_history on the host: V0, then p.iterations iterations.  Returns (status, V0, [(colour, variance) after each iteration])"""
    rc, v0 = variance(hist.colour, hist.length, hist.moments, guides, p, L)
    if rc != 0:
        return rc, None, None
    c, v, steps = hist.colour, v0, []
    for i in range(p.iterations):
        rc, c, v = iteration(c, v, guides, p, i, L)
        assert rc == 0
        steps.append((c, v))
    return 0, v0, steps


def constants(p, planes=0, L=None):
    """(status, reason)"""
    why = C.create_string_buffer(128)
    rc = (L or lib()).sh_constants(None if p is None else C.byref(p), planes, why, 128)
    return rc, why.value.decode()
