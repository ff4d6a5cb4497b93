"""The host build of the temporal stage (tests/cpp/temporal_host.cpp: vk_raytrace_amd/csrc/pt_temporal.h compiled by g++) and its Python side.  The
library is one of host_harness.build_library's, cached under tests/cpp/_build/; it needs no libptmi.so.  A plain module: no test lives here."""
import ctypes as C

import numpy as np

from tests import host_harness as hh
from vk_raytrace_amd import host_device as hd

CSRC, COMPILE = hh.CSRC, hh.COMPILE   # where the header lies and what it is compiled with, for the tests that plant a break in a scratch copy
_P = C.c_void_p
_CALL = [_P, _P, _P, C.c_int, C.c_int, _P, _P, C.POINTER(hd.TemporalParams), _P, _P, _P, _P, _P]
SIGNATURES = [
    ("th_temporal", C.c_int, _CALL + [_P, _P, _P]),
    ("th_temporal_probe", C.c_int, _CALL + [_P, _P, _P, _P, _P, _P]),
    ("th_temporal_constants", C.c_int, [C.POINTER(hd.TemporalParams), C.c_char_p, C.c_int]),
]
# TemporalProbe::verdict and the outcomes of step 4 (csrc/pt_temporal.h)
COUNTED, OUTSIDE, TOO_SHORT, NOT_FINITE, DEPTH, NORMAL = 1, 2, 3, 4, 5, 6
BLEND, HISTORY_ONLY, CURRENT, NOTHING = 0, 1, 2, 3
_host = hh.StageLibrary("libtemporalhost", "temporal_host.cpp", SIGNATURES)
build, compile_to, bind, lib = _host.build, _host.compile_to, _host.bind, _host.lib


def params(world_to_clip, depth_tol, normal_dist2, max_history, flags=0):
    p = hd.TemporalParams(depthTol=depth_tol, normalDist2=normal_dist2, maxHistory=max_history, flags=flags)
    C.memmove(p.worldToClip, np.ascontiguousarray(world_to_clip, np.float32).ctypes.data, 64)   # bit patterns as given (NaN payloads included)
    return p


class History:
    """what a call leaves for the next: the three images and the camera they were made with"""
    def __init__(self, colour, guide, length, world_to_clip, eye):
        self.colour, self.guide, self.length = colour, guide, length
        self.world_to_clip, self.eye = np.ascontiguousarray(world_to_clip, np.float32).reshape(16), np.ascontiguousarray(eye, np.float32).reshape(3)


def _inputs(colour, normal, depth, view_inverse, proj_inverse, hist):
    colour = np.ascontiguousarray(colour, np.float32)
    h, w = colour.shape[:2]
    normal, depth = np.ascontiguousarray(normal, np.float32), np.ascontiguousarray(depth, np.float32)
    assert normal.shape == colour.shape == depth.shape == (h, w, 4)
    vi, pi = np.ascontiguousarray(view_inverse, np.float32).reshape(16), np.ascontiguousarray(proj_inverse, np.float32).reshape(16)
    keep = [colour, normal, depth, vi, pi]
    if hist is None:
        tail = [None] * 5
    else:
        hc, hg, hn = (np.ascontiguousarray(a, np.float32) for a in (hist.colour, hist.guide, hist.length))
        assert hc.shape == (h, w, 4) == hg.shape and hn.shape == (h, w)
        keep += [hc, hg, hn, hist.world_to_clip, hist.eye]
        tail = [a.ctypes.data for a in keep[5:]]
    return w, h, keep, [colour.ctypes.data, normal.ctypes.data, depth.ctypes.data, w, h, vi.ctypes.data, pi.ctypes.data], tail


def temporal(colour, normal, depth, view_inverse, proj_inverse, p, hist=None, L=None):
    """th_temporal: one call.  Returns (status, History or None): the new history, made with p.worldToClip and the eye of view_inverse"""
    w, h, keep, head, tail = _inputs(colour, normal, depth, view_inverse, proj_inverse, hist)
    oc, og, on = np.empty((h, w, 4), np.float32), np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32)
    rc = (L or lib()).th_temporal(*head, C.byref(p), *tail, oc.ctypes.data, og.ctypes.data, on.ctypes.data)
    if rc != 0:
        return rc, None
    return rc, History(oc, og, on, np.array(p.worldToClip, np.float32), keep[3][12:15])


def probe(colour, normal, depth, view_inverse, proj_inverse, p, hist=None, L=None):
    """th_temporal_probe: dict of fxfy (H, W, 2), taps (H, W, 4, 2), verdicts (H, W, 4), sw, outcome (H, W), point (H, W, 4: P.xyz, t_exp)"""
    w, h, keep, head, tail = _inputs(colour, normal, depth, view_inverse, proj_inverse, hist)
    out = {"fxfy": np.empty((h, w, 2), np.float32), "taps": np.empty((h, w, 4, 2), np.int32), "verdicts": np.empty((h, w, 4), np.int32),
           "sw": np.empty((h, w), np.float32), "outcome": np.empty((h, w), np.int32), "point": np.empty((h, w, 4), np.float32)}
    rc = (L or lib()).th_temporal_probe(*head, C.byref(p), *tail, *[out[k].ctypes.data for k in ("fxfy", "taps", "verdicts", "sw", "outcome", "point")])
    assert rc == 0, rc
    return out


def constants(p, L=None):
    """(status, reason)"""
    why = C.create_string_buffer(128)
    rc = (L or lib()).th_temporal_constants(None if p is None else C.byref(p), why, 128)
    return rc, why.value.decode()
