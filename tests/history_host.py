"""One call of the history stage on the host (tests/cpp/stage/history_step.h), from Python: the record the step entries of the five history libraries
take (temporal_host, svgf_host, motion_host, albedo_host, fast_host), the history a call leaves, and the one function that prepares the arrays, calls an
entry and builds that history.  A plain module: no test lives here."""
import ctypes as C

import numpy as np

from vk_raytrace_amd import host_device as hd

_P = C.c_void_p
PROBES = ("fxfy", "taps", "verdicts", "sw", "outcome", "point")     # per pixel: (2) f32, (4, 2) i32, (4) i32, () f32, () i32, (4) f32


class Call(C.Structure):
    """HistoryCall, field for field (every stage library's hs_call_layout says where the compiler put them)"""
    _fields_ = ([(n, _P) for n in ("colour", "albedo", "normal", "depth")] + [("w", C.c_int), ("h", C.c_int), ("view_inverse", _P), ("proj_inverse", _P),
                ("params", C.POINTER(hd.TemporalParams))]
                + [(n, _P) for n in ("hist_colour", "hist_guide", "hist_length", "hist_moments", "hist_fast", "hist_fast_length", "world_to_clip_h", "eye_h", "ids", "table")]
                + [("num_instances", C.c_uint32), ("fast", C.POINTER(hd.FastParams))]
                + [(n, _P) for n in ("out_colour", "out_guide", "out_length", "out_moments", "out_fast", "out_fast_length", "unclamped") + PROBES])


STEP = [C.POINTER(Call)]                                                   # the argtypes of every step entry
LAYOUT = ("hs_call_layout", C.c_int, [C.POINTER(C.c_size_t), C.c_int])     # the signature-table line of the entry every stage library exports


def layout(L):
    """hs_call_layout of the bound library L: [sizeof(HistoryCall), the offset of each field in declaration order]"""
    out = (C.c_size_t * 64)()
    return list(out[:L.hs_call_layout(out, 64)])


class History:
    """what a call leaves for the next: the images and the camera they were made with.  moments: with tracking on; fast, fast_length: with
    pt_temporal_fast on, and then raw, raw_length: the long step's result before the clamp, for the tests"""
    def __init__(self, colour, guide, length, world_to_clip, eye, moments=None, fast=None, fast_length=None, raw=None, raw_length=None):
        self.colour, self.guide, self.length, self.moments = colour, guide, length, moments
        self.world_to_clip, self.eye = np.ascontiguousarray(world_to_clip, np.float32).reshape(16), np.ascontiguousarray(eye, np.float32).reshape(3)
        self.fast, self.fast_length, self.raw, self.raw_length = fast, fast_length, raw, raw_length


def run(entry, colour, normal, depth, view_inverse, proj_inverse, p, hist=None, albedo=None, ids=None, tab=None, fp=None, moments=False, images=True, probes=()):
    """One call of the step entry `entry` (a bound function).  albedo None: pt_temporal_demodulate off.  ids None: the static form; else (H, W) uint32
    with tab what motion_host.table returns (None: no instances).  fp None: pt_temporal_fast off.  moments: the history (if any) has .moments and the new
    one gets them.  images: the new history is asked for.  probes: the names among PROBES to hand out.
    Returns (status, History or None -- made with p.worldToClip and the eye of view_inverse --, {name: array} of the probes)"""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)   # noqa: E731
    colour = f32(colour)
    h, w = colour.shape[:2]
    q, keep = Call(w=w, h=h, params=C.pointer(p), fast=None if fp is None else C.pointer(fp)), []

    def put(name, a, shape, dtype=np.float32):
        a = np.ascontiguousarray(a, dtype)
        assert a.shape == shape, (name, a.shape, shape)
        keep.append(a)
        setattr(q, name, a.ctypes.data)
        return a

    def out(name, shape, dtype=np.float32):
        return put(name, np.empty(shape, dtype), shape, dtype)

    put("colour", colour, (h, w, 4)), put("normal", normal, (h, w, 4)), put("depth", depth, (h, w, 4))
    eye = put("view_inverse", f32(view_inverse).reshape(16), (16,))[12:15]
    put("proj_inverse", f32(proj_inverse).reshape(16), (16,))
    if albedo is not None:
        put("albedo", albedo, (h, w, 4))
    if ids is not None:
        put("ids", ids, (h, w), np.uint32)
    if tab is not None:
        q.num_instances = len(put("table", tab, np.shape(tab)))
    if hist is not None:
        put("hist_colour", hist.colour, (h, w, 4)), put("hist_guide", hist.guide, (h, w, 4)), put("hist_length", hist.length, (h, w))
        put("world_to_clip_h", hist.world_to_clip, (16,)), put("eye_h", hist.eye, (3,))
        if moments:
            put("hist_moments", hist.moments, (h, w, 2))
        if fp is not None:
            put("hist_fast", hist.fast, (h, w, 4)), put("hist_fast_length", hist.fast_length, (h, w))
    new = {}
    if images:
        new = {"colour": out("out_colour", (h, w, 4)), "guide": out("out_guide", (h, w, 4)), "length": out("out_length", (h, w))}
        if moments:
            new["moments"] = out("out_moments", (h, w, 2))
        if fp is not None:
            new["fast"], new["fast_length"], raw = out("out_fast", (h, w, 4)), out("out_fast_length", (h, w)), out("unclamped", (h * w * 5,))
    shapes = {"fxfy": ((h, w, 2), np.float32), "taps": ((h, w, 4, 2), np.int32), "verdicts": ((h, w, 4), np.int32), "sw": ((h, w), np.float32),
              "outcome": ((h, w), np.int32), "point": ((h, w, 4), np.float32)}
    looked = {name: out(name, *shapes[name]) for name in probes}
    rc = entry(C.byref(q))
    if rc != 0 or not images:
        return rc, None, looked
    if fp is not None:
        new["raw"], new["raw_length"] = raw[:h * w * 4].reshape(h, w, 4).copy(), raw[h * w * 4:].reshape(h, w).copy()
    return rc, History(world_to_clip=np.array(p.worldToClip, np.float32), eye=eye, **new), looked
