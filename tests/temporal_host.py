"""The host build of the temporal stage (tests/cpp/temporal_host.cpp: vk_raytrace_amd/csrc/pt_temporal.h compiled by g++) and its Python side.  The
library is one of host_harness.build_library's, cached under tests/cpp/_build/; it needs no libptmi.so.  A plain module: no test lives here."""
import ctypes as C

import numpy as np

from tests import history_host as hs, host_harness as hh
from vk_raytrace_amd import host_device as hd

CSRC, COMPILE = hh.CSRC, hh.COMPILE   # where the header lies and what it is compiled with, for the tests that plant a break in a scratch copy
SIGNATURES = [
    ("th_temporal", C.c_int, hs.STEP),
    ("th_temporal_constants", C.c_int, [C.POINTER(hd.TemporalParams), C.c_char_p, C.c_int]),
    hs.LAYOUT,
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


History = hs.History     # colour, guide, length, world_to_clip, eye


def temporal(colour, normal, depth, view_inverse, proj_inverse, p, hist=None, L=None):
    """th_temporal: one call.  Returns (status, History or None): the new history, made with p.worldToClip and the eye of view_inverse"""
    return hs.run((L or lib()).th_temporal, colour, normal, depth, view_inverse, proj_inverse, p, hist)[:2]


def probe(colour, normal, depth, view_inverse, proj_inverse, p, hist=None, L=None):
    """th_temporal, looked into: dict of fxfy (H, W, 2), taps (H, W, 4, 2), verdicts (H, W, 4), sw, outcome (H, W), point (H, W, 4: P.xyz, t_exp)"""
    rc, _, out = hs.run((L or lib()).th_temporal, colour, normal, depth, view_inverse, proj_inverse, p, hist, images=False, probes=hs.PROBES)
    assert rc == 0, rc
    return out


def constants(p, L=None):
    """(status, reason)"""
    why = C.create_string_buffer(128)
    rc = (L or lib()).th_temporal_constants(None if p is None else C.byref(p), why, 128)
    return rc, why.value.decode()
