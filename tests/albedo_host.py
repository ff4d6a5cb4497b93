"""The host build of the demodulated history (tests/cpp/albedo_host.cpp: vk_raytrace_amd/csrc/pt_albedo.h in front of pt_temporal.h, pt_motion.h and
pt_svgf.h, compiled by g++) and its Python side.  The library is one of host_harness.build_library's, cached under
tests/cpp/_build/; it needs no libptmi.so.  A plain module: no test lives here."""
import ctypes as C

import numpy as np

from tests import history_host as hs, host_harness as hh, svgf_host as sh

CSRC, COMPILE = hh.CSRC, hh.COMPILE
_P = C.c_void_p
SIGNATURES = [
    ("ah_temporal", C.c_int, hs.STEP),
    ("ah_remodulate", None, [_P, _P, C.c_size_t, _P]),
    ("ah_refusal", C.c_int, [C.c_int, C.c_int, C.c_uint32, C.c_char_p, C.c_int]),
    hs.LAYOUT,
]
SETTING, STEP_NEEDS_PLANE, NEED_PLANE, DENOISE_FLAGS = 0, 1, 2, 3   # ah_refusal's `what`
_host = hh.StageLibrary("libalbedohost", "albedo_host.cpp", SIGNATURES)
build, compile_to, bind, lib = _host.build, _host.compile_to, _host.bind, _host.lib
History = hs.History     # colour, guide, length, world_to_clip, eye and .moments (None: not tracked)


def temporal(colour, albedo, normal, depth, view_inverse, proj_inverse, p, hist=None, moments=False, ids=None, tab=None, want_outcome=False, L=None):
    """ah_temporal: one call of the demodulating step.  ids None: the static form; else (H, W) uint32 with tab what motion_host.table returns.
    moments: the history (if any) has .moments and the new one gets them.  Returns (status, History or None[, outcome (H, W) int32])"""
    rc, new, pr = hs.run((L or lib()).ah_temporal, colour, normal, depth, view_inverse, proj_inverse, p, hist, albedo=albedo, ids=ids, tab=tab, moments=moments,
                         probes=("outcome",) if want_outcome else ())
    return (rc, new, pr["outcome"]) if want_outcome else (rc, new)


def remodulate(x, albedo, L=None):
    """ah_remodulate: x * max(albedo, floor) per pixel, (H, W, 4) float32"""
    a, g = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(albedo, np.float32)
    assert a.shape == g.shape and a.shape[-1] == 4
    out = np.empty_like(a)
    (L or lib()).ah_remodulate(a.ctypes.data, g.ctypes.data, a.size // 4, out.ctypes.data)
    return out


def refusal(what, a, b=0, L=None):
    """(status, reason) of one of pt_albedo.h's refusals"""
    why = C.create_string_buffer(160)
    rc = (L or lib()).ah_refusal(what, int(a), int(b), why, 160)
    return rc, why.value.decode()


def svgf_history(hist, guides, p, L=None, sL=None):
    """pt_svgf_history on a demodulated history, on the host: svgf_host.filter_history as it stands, then the remodulation of the last iteration's image
    by guides[0].  Returns (status, image (H, W, 4), variance after the last iteration (H, W) -- in demodulated units)"""
    rc, _, steps = sh.filter_history(sh.History(hist.colour, hist.guide, hist.length, hist.moments, hist.world_to_clip, hist.eye), guides, p, sL)
    if rc != 0:
        return rc, None, None
    return 0, remodulate(steps[-1][0], guides[0], L), steps[-1][1]
