"""Time of the temporal reprojection stage (pt_temporal_accumulate) on the Sponza stand-in (workloads C3) at 1920x1080 after a real camera move, against
its traffic floor at the HBM streaming rate measured in the same run:

    python tools/temporal_rate.py > profiles/temporal_rate.txt

Set-up: camera A, pt_render_guides(7), one frame-0 1 spp frame, pt_temporal_accumulate (the history); then camera B -- a dolly, a strafe and a yaw of
the workload's camera, so that the gather is a real reprojection with disocclusions -- guides and a frame again.  The stage alone is then timed with
device events (pt_debug_temporal_time: the kernel enqueued 50 times between two events after a warm-up run, reading the history and writing the other
set; no untile pass, no copy), three rounds, the median printed; the same with a static camera (history made with B) and for a first call (no
history) next to it.  The host-side cost of the synchronous entry point is reported separately: pt_temporal_accumulate with its image copied out
against pt_read_accum (both end in the copy of the 33 MB image to pageable host memory), and without the copy, median of 10 calls.

Traffic floor, at pt_measure_peaks' float4 copy rate (read + written bytes per second): 136 bytes per pixel is the figure the stage was specified against.
The planes this kernel moves sum to 120: reads of the colour and the two guide planes (48), one read of the history's colour, guide and length (36;
the four taps of neighbouring pixels overlap) and writes of the new three (36) -- it writes no result image of its own, the new history colour IS
the result.  Both ratios are printed.  A measurement, not a threshold."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vk_raytrace_amd import capi, host_device as hd, workloads  # noqa: E402
from vk_raytrace_amd.renderer import HipRenderer  # noqa: E402
from vk_raytrace_amd.scene import Camera  # noqa: E402

W, H, REPS, ROUNDS = 1920, 1080, 50, 3
MISS_DEPTH = 1.0e4   # finite and far below 1e18: the sky keeps its history under rotation
FLOOR_BYTES = 136    # per pixel: the floor the stage was specified against
KERNEL_BYTES = 120   # ... what k_temporal must move: 48 read (colour, normal, depth planes) + 36 read (history) + 36 written


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


def stage_ms(r, p):
    ms = C.c_float()
    r._check(capi.lib().pt_debug_temporal_time(r._ctx, C.byref(p), REPS, C.byref(ms)))
    return ms.value


def host_ms(fn, n=10):
    fn()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    wl = workloads.c3_sponza(W, H, 1)
    if wl.scene.vertices is None:
        wl.scene.finalize(capi.pack_vertices)
    print(f"{wl.name}; library {os.path.relpath(capi.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))}")
    r = HipRenderer()
    r.setup(0)
    r.set_scene(wl.scene)
    integral, _ = r.set_env(wl.env)
    r.set_sunsky(hd.default_sun_and_sky())
    r.create((W, H))
    st = hd.default_rtx_state()
    st.size[0], st.size[1] = W, H
    st.maxDepth, st.pbrMode, st.fireflyClampThreshold, st.frame = wl.depth, wl.pbr_mode, 4.0 * integral, 0

    def frame_at(cam):
        r.set_camera(capi.camera_lookat(cam, W / H, nb_lights=len(wl.scene.lights)))
        r.capture_guides(7, MISS_DEPTH)
        r.setPushContants(st)
        r.run()
        return r.temporal_params(r.world_to_clip(cam, W / H), 0.05, 0.05, 32.0)

    cam_a, cam_b = wl.scene.camera, moved(wl.scene.camera)
    table = {}
    for _ in range(ROUNDS):
        r.temporal_reset()
        p_a = frame_at(cam_a)
        table.setdefault("first call (no history)", []).append(stage_ms(r, p_a))
        r.temporal_accumulate(p_a, read=False)
        p_b = frame_at(cam_b)
        table.setdefault("after the camera move", []).append(stage_ms(r, p_b))
        r.temporal_accumulate(p_b, read=False)
        _, length = r.read_temporal_history()
        table.setdefault("static camera", []).append(stage_ms(r, p_b))
    peaks = r.measure_peaks()
    copy_rate = peaks["hbmCopyBytesPerSec"]
    floor_ms = FLOOR_BYTES * W * H / copy_rate * 1e3
    print(f"{W}x{H}; HBM float4 copy {copy_rate / 1e12:.2f} TB/s, read {peaks['hbmReadBytesPerSec'] / 1e12:.2f} TB/s (pt_measure_peaks, this run); traffic floor "
          f"{FLOOR_BYTES} B per pixel = {FLOOR_BYTES * W * H / 1e6:.0f} MB = {floor_ms:.3f} ms at the copy rate")
    print(f"after the move {100.0 * float((length > 1).mean()):.1f} % of the pixels found history (length > 1)")
    for name, v in table.items():
        med = statistics.median(v)
        print(f"k_temporal, {name}: {med:.3f} ms = {med / floor_ms:.2f} x the floor ({med / (floor_ms * KERNEL_BYTES / FLOOR_BYTES):.2f} x the {KERNEL_BYTES} B the kernel must move)   [rounds: {' '.join(f'{x:.3f}' for x in v)}]")
    a = host_ms(r.read_accum)
    b = host_ms(lambda: r.temporal_accumulate(p_b))
    c = host_ms(lambda: r.temporal_accumulate(p_b, read=False))
    print(f"host clock, synchronous calls: pt_read_accum {a[0]:.2f} ms, pt_temporal_accumulate with its image copied out {b[0]:.2f} ms (difference {b[0] - a[0]:.2f} ms), "
          f"without the copy {c[0]:.3f} ms (min {c[1]:.3f}, max {c[2]:.3f})")
    r.destroy()


if __name__ == "__main__":
    main()
