"""What the rate tools of the display stages (denoise_rate.py, guides_rate.py, temporal_rate.py, svgf_rate.py) share: the renderer on the Sponza stand-in
(workloads C3), a frame and its guide planes at a camera, the tools' standard camera move, the call of a pt_debug_*_time entry, the host-clock timing of a
synchronous call and the way medians and rounds are printed.  A plain module: it measures nothing by itself."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vk_raytrace_amd import capi, host_device as hd, workloads  # noqa: E402
from vk_raytrace_amd.renderer import HipRenderer  # noqa: E402
from vk_raytrace_amd.scene import Camera  # noqa: E402

REPS, ROUNDS = 50, 3   # runs between the two events of a pt_debug_*_time call; rounds a tool alternates its choices over
MISS_DEPTH = 1.0e4     # finite and far below 1e18: the sky keeps its history under rotation


def c3_workload(w, h):
    """the workload, its scene finalized; prints the line every record under profiles/ starts with"""
    wl = workloads.c3_sponza(w, h, 1)
    if wl.scene.vertices is None:
        wl.scene.finalize(capi.pack_vertices)
    print(f"{wl.name}; library {os.path.relpath(capi.LIB_PATH, ROOT)}")
    return wl


def c3_renderer(w, h):
    """(workload, renderer with its scene, environment and image, the push constants of a 1 spp frame 0)"""
    wl = c3_workload(w, h)
    r = HipRenderer()
    r.setup(0)
    r.set_scene(wl.scene)
    integral, _ = r.set_env(wl.env)
    r.set_sunsky(hd.default_sun_and_sky())
    r.create((w, h))
    st = hd.default_rtx_state()
    st.size[0], st.size[1] = w, h
    st.maxDepth, st.pbrMode, st.fireflyClampThreshold, st.frame = wl.depth, wl.pbr_mode, 4.0 * integral, 0
    return wl, r, st


def frame_at(r, wl, st, cam):
    """the camera set, its guide planes and one frame rendered: the parameters of a pt_temporal_accumulate there"""
    w, h = st.size[0], st.size[1]
    r.set_camera(capi.camera_lookat(cam, w / h, nb_lights=len(wl.scene.lights)))
    r.capture_guides(7, MISS_DEPTH)
    r.setPushContants(st)
    r.run()
    return r.temporal_params(r.world_to_clip(cam, w / h), 0.05, 0.05, 32.0)


def moved(cam):
    """the workload's camera after a dolly of 5 % of its focus distance, a strafe of half that and a yaw of 2 degrees"""
    eye, center = np.array(cam.eye, np.float64), np.array(cam.center, np.float64)
    fwd = center - eye
    dist = np.linalg.norm(fwd)
    fwd /= dist
    right = np.cross(fwd, np.array(cam.up, np.float64))
    right /= np.linalg.norm(right)
    eye2 = eye + 0.05 * dist * fwd + 0.025 * dist * right
    a = np.radians(2.0)
    d = center - eye
    d = np.array([np.cos(a) * d[0] + np.sin(a) * d[2], d[1], -np.sin(a) * d[0] + np.cos(a) * d[2]])
    return Camera(eye=tuple(eye2), center=tuple(eye2 + d), up=cam.up, fov=cam.fov)


def stage_ms(r, fn_name, *args):
    """pt_debug_<stage>_time(ctx, *args, REPS, &ms): milliseconds per run, by device events"""
    ms = C.c_float()
    r._check(getattr(capi.lib(), fn_name)(r._ctx, *args, REPS, C.byref(ms)))
    return ms.value


def host_ms(fn, n=10):
    """(median, min, max) milliseconds of n calls by the host clock, after one call that is not counted"""
    fn()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def rounds(v):
    return f"[rounds: {' '.join(f'{x:.3f}' for x in v)}]"


def med(v):
    return f"{statistics.median(v):.3f} ms {rounds(v)}"
