"""The host build of the motion of moving instances (tests/cpp/motion_host.cpp: vk_raytrace_amd/csrc/pt_motion.h and instance_pixel of pt_guides.h
compiled by g++) and its Python side.  The library is one of host_harness.build_library's, cached under tests/cpp/_build/; it
needs no libptmi.so.  The instance pass works on the scene handle a host_harness.TracedScene holds, with the camera guides_host.set_camera gave it.
A plain module: no test lives here."""
import ctypes as C

import numpy as np

from tests import history_host as hs, host_harness as hh

CSRC, COMPILE = hh.CSRC, hh.COMPILE
_P = C.c_void_p
SIGNATURES = [
    ("mh_table", None, [_P, _P, C.c_uint32, _P]),
    ("mh_temporal_moving", C.c_int, hs.STEP),
    ("mh_instances", C.c_uint32, [_P, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_float, _P, _P, _P, _P]),
    hs.LAYOUT,
]
INSTANCE_WORDS = 24     # PT_MOTION_INSTANCE_WORDS: objectToWorld rows (12), worldToObject rows (12)
RECORD_WORDS = 28       # MotionRec: toPrev rows (12), normalToPrev rows (12), moved, padding (3)
NONE = 0xFFFFFFFF
_host = hh.StageLibrary("libmotionhost", "motion_host.cpp", SIGNATURES)
build, compile_to, bind, lib = _host.build, _host.compile_to, _host.bind, _host.lib


def instance_words(world):
    """The words pt_set_scene / pt_update_instances keep per node for a 4 x 4 world matrix given as a mathematical (row, column) array -- what
    vk_raytrace_amd/csrc/pt_scene_records.cpp instance_transform does: the fp32 matrix's three rows, and the rows of its inverse formed in double from
    the fp32 words and rounded once"""
    m = np.asarray(world, np.float32)
    (a, b, c, tx), (d, e, f, ty), (g, h, i, tz) = [[float(v) for v in row] for row in m[:3]]
    A, B, Cc = e * i - f * h, -(d * i - f * g), d * h - e * g       # its cofactor expansion, statement by statement (Python floats are doubles)
    r = 1.0 / (a * A + b * B + c * Cc)
    i00, i01, i02 = A * r, -(b * i - c * h) * r, (b * f - c * e) * r
    i10, i11, i12 = B * r, (a * i - c * g) * r, -(a * f - c * d) * r
    i20, i21, i22 = Cc * r, -(a * h - b * g) * r, (a * e - b * d) * r
    inv = [i00, i01, i02, -(i00 * tx + i01 * ty + i02 * tz), i10, i11, i12, -(i10 * tx + i11 * ty + i12 * tz), i20, i21, i22, -(i20 * tx + i21 * ty + i22 * tz)]
    return np.concatenate([m[:3].reshape(12), np.array(inv, np.float64).astype(np.float32)]).astype(np.float32)


def table(hist_words, cur_words, L=None):
    """mh_table: (n, 28) float32 records (word 24 viewed as uint32 is `moved`) from two (n, 24) arrays of instance words"""
    a, b = np.ascontiguousarray(hist_words, np.float32).reshape(-1, INSTANCE_WORDS), np.ascontiguousarray(cur_words, np.float32).reshape(-1, INSTANCE_WORDS)
    assert a.shape == b.shape
    out = np.zeros((len(a), RECORD_WORDS), np.float32)
    (L or lib()).mh_table(a.ctypes.data, b.ctypes.data, len(a), out.ctypes.data)
    return out


def moved_bits(tab):
    return np.ascontiguousarray(tab[:, 24]).view(np.uint32)


History = hs.History     # colour, guide, length, world_to_clip, eye and .moments (None: not tracked)


def temporal_moving(colour, normal, depth, view_inverse, proj_inverse, p, ids, tab, hist=None, moments=False, want_probe=False, L=None):
    """mh_temporal_moving: one call.  ids: (H, W) uint32; tab: what table() returns (None: no instances).  Returns (status, History or None[, probe dict
    as temporal_host.probe returns it, its point being (P'.xyz, t_exp)])"""
    rc, new, pr = hs.run((L or lib()).mh_temporal_moving, colour, normal, depth, view_inverse, proj_inverse, p, hist, ids=ids, tab=tab, moments=moments,
                         probes=hs.PROBES if want_probe else ())
    return (rc, new, pr) if want_probe else (rc, new)


def instances(traced, two, width, height, planes=0, miss_depth=1.0e30):
    """mh_instances: (ids (H, W) uint32, the three guide planes -- None outside `planes`) of the scene `traced` holds for the camera
    guides_host.set_camera gave it"""
    ids = np.zeros((height, width), np.uint32)
    out = [np.zeros((height, width, 4), np.float32) if planes & (1 << j) else None for j in range(3)]
    over = lib().mh_instances(traced.h, int(two), width, height, planes, miss_depth, ids.ctypes.data, *[None if p is None else p.ctypes.data for p in out])
    assert over == 0, "traversal stack overflow"
    return ids, tuple(out)
