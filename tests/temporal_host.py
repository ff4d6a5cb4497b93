"""The host build of the temporal stage (tests/cpp/temporal_host.cpp: vk_raytrace_amd/csrc/pt_temporal.h compiled by g++) and its Python side.  A
library of its own with its own g++ call -- the compile flags are denoise_host's -- cached under tests/cpp/_build/.  A plain module: no test lives
here."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from vk_raytrace_amd import host_device as hd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vk_raytrace_amd", "csrc")
BUILD_DIR = os.path.join(CPP, "_build")
OUT = os.path.join(BUILD_DIR, "libtemporalhost.so")
SOURCES = [os.path.join(CPP, "temporal_host.cpp"), os.path.join(CSRC, "pt_temporal.h"), os.path.join(CSRC, "pt_denoise.h"), os.path.join(ROOT, "include", "pt_fpmath.h"),
           os.path.join(ROOT, "include", "pt_types.h"), os.path.join(ROOT, "include", "pt_api.h")]
COMPILE = ["-std=c++17", "-O2", "-fopenmp", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-DSTACK_LDS=24", "-Wno-attributes",
           "-I/opt/rocm/include", "-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
_lib = None

# TemporalProbe::verdict and the outcomes of step 4 (csrc/pt_temporal.h)
COUNTED, OUTSIDE, TOO_SHORT, NOT_FINITE, DEPTH, NORMAL = 1, 2, 3, 4, 5, 6
BLEND, HISTORY_ONLY, CURRENT, NOTHING = 0, 1, 2, 3


def compile_to(out, header_dir=None):
    """g++ of temporal_host.cpp to `out`; header_dir: a directory searched before csrc/ (a scratch copy of pt_temporal.h with a planted break)"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    fd, tmp = tempfile.mkstemp(suffix=".so", dir=os.path.dirname(out))   # concurrent builders each write a file of their own; nobody loads a half-written one
    os.close(fd)
    try:
        subprocess.check_call(["g++"] + ([] if header_dir is None else ["-I" + header_dir]) + COMPILE + ["-shared", "-o", tmp, SOURCES[0]])
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return out


def build():
    """libtemporalhost.so, compiled if it is missing or older than a source it is made of; returns its path"""
    if os.path.exists(OUT) and all(os.path.getmtime(s) <= os.path.getmtime(OUT) for s in SOURCES + [os.path.abspath(__file__)]):
        return OUT
    return compile_to(OUT)


_P = C.c_void_p
_CALL = [_P, _P, _P, C.c_int, C.c_int, _P, _P, C.POINTER(hd.TemporalParams), _P, _P, _P, _P, _P]


def bind(path):
    L = C.CDLL(path)
    L.th_temporal.restype, L.th_temporal.argtypes = C.c_int, _CALL + [_P, _P, _P]
    L.th_temporal_probe.restype, L.th_temporal_probe.argtypes = C.c_int, _CALL + [_P, _P, _P, _P, _P, _P]
    L.th_temporal_constants.restype, L.th_temporal_constants.argtypes = C.c_int, [C.POINTER(hd.TemporalParams), C.c_char_p, C.c_int]
    return L


def lib():
    global _lib
    if _lib is None:
        _lib = bind(build())
    return _lib


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
