"""The host build of the responsive history (tests/cpp/fast_host.cpp: vk_raytrace_amd/csrc/pt_fast.h behind the temporal steps of pt_temporal.h,
pt_motion.h, pt_albedo.h and pt_svgf.h, compiled by g++) and its Python side.  The library is one of
host_harness.build_library's, cached under tests/cpp/_build/; it needs no libptmi.so.  A plain module: no test lives here."""
import ctypes as C

import numpy as np

from tests import history_host as hs, host_harness as hh
from vk_raytrace_amd import host_device as hd

CSRC, COMPILE = hh.CSRC, hh.COMPILE
_P = C.c_void_p
_FP = C.POINTER(hd.FastParams)
SIGNATURES = [
    ("fh_constants", C.c_int, [_FP, C.c_char_p, C.c_int]),
    ("fh_need_history", C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    ("fh_clamp", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _FP] + [_P] * 8),
    ("fh_step", C.c_int, hs.STEP),
    hs.LAYOUT,
]
_host = hh.StageLibrary("libfasthost", "fast_host.cpp", SIGNATURES)
build, compile_to, bind, lib = _host.build, _host.compile_to, _host.bind, _host.lib


def params(max_fast=4.0, sigma_scale=2.0, radius=2, flags=0):
    return hd.FastParams(maxFast=max_fast, sigmaScale=sigma_scale, radius=radius, flags=flags)


History = hs.History     # ... with the fast images (fast, fast_length) and, for the tests, the long step's result before the clamp (raw, raw_length)


def constants(p, L=None):
    """(status, reason) of fast_constants"""
    why = C.create_string_buffer(160)
    rc = (L or lib()).fh_constants(None if p is None else C.byref(p), why, 160)
    return rc, why.value.decode()


def need_history(hist_fast, L=None):
    why = C.create_string_buffer(160)
    rc = (L or lib()).fh_need_history(int(hist_fast), why, 160)
    return rc, why.value.decode()


def clamp(hf, hnf, hc, hn, fp, want_probe=False, L=None):
    """fh_clamp: the clamp alone.  Returns (status, colour (H, W, 4), length (H, W)[, probe dict: n (H, W), mu / sigma / lo / hi (H, W, 3), moved (H, W)])"""
    hf, hc = np.ascontiguousarray(hf, np.float32), np.ascontiguousarray(hc, np.float32)
    hnf, hn = np.ascontiguousarray(hnf, np.float32), np.ascontiguousarray(hn, np.float32)
    h, w = hn.shape
    assert hf.shape == hc.shape == (h, w, 4) and hnf.shape == (h, w)
    oc, on = np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32)
    pr = {"n": np.empty((h, w), np.float32), "mu": np.empty((h, w, 3), np.float32), "sigma": np.empty((h, w, 3), np.float32), "lo": np.empty((h, w, 3), np.float32),
          "hi": np.empty((h, w, 3), np.float32), "moved": np.empty((h, w), np.int32)}
    rc = (L or lib()).fh_clamp(hf.ctypes.data, hnf.ctypes.data, hc.ctypes.data, hn.ctypes.data, w, h, C.byref(fp), oc.ctypes.data, on.ctypes.data,
                               *[pr[k].ctypes.data for k in ("n", "mu", "sigma", "lo", "hi", "moved")])
    if rc != 0:
        return (rc, None, None, None) if want_probe else (rc, None, None)
    return (rc, oc, on, pr) if want_probe else (rc, oc, on)


def step(colour, albedo, normal, depth, view_inverse, proj_inverse, p, fp, hist=None, moments=False, ids=None, tab=None, L=None):
    """fh_step: one call with the setting on.  albedo None: pt_temporal_demodulate off.  ids None: the static form; else (H, W) uint32 with tab what
    motion_host.table returns.  hist: a History of this module (or None).  Returns (status, History or None)"""
    return hs.run((L or lib()).fh_step, colour, normal, depth, view_inverse, proj_inverse, p, hist, albedo=albedo, ids=ids, tab=tab, fp=fp, moments=moments)[:2]
