"""Time of the two kernels the motion of moving instances adds on the Sponza stand-in (workloads C3) at 1920x1080, each against
the kernel it stands in for, timed in the same run:

    python tools/motion_rate.py > profiles/motion_rate.txt

k_instances (pt_render_instance_plane) against k_guides (pt_render_guides), all three guide planes, and with a mask of 0: it moves 52 B per pixel against
48 B, and the first-hit walk dominates both.  k_temporal_moving (pt_temporal_accumulate_moving) against k_temporal (pt_temporal_accumulate) after the
camera move of tools/temporal_rate.py with one node of the scene moved besides -- the node that covers the most pixels among those that cover less than
a quarter of the image, translated by 2 % of the camera's focus distance -- with pt_temporal_track_moments off and on: it moves 4 B more than the 120 B
(136 B with moments) per pixel, and the table's records of the pixels that moved.  Device events (pt_debug_guides_time, pt_debug_temporal_time,
pt_debug_motion_time: the kernel enqueued 50 times between two events after a warm-up run), three rounds in which the kernels alternate, the median and
the rounds printed; the HBM float4 copy rate of pt_measure_peaks in the same run beside them.  A measurement, not a threshold."""
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rate_common import MISS_DEPTH, ROUNDS, c3_renderer, frame_at, moved, rounds, stage_ms  # noqa: E402
from vk_raytrace_amd import capi  # noqa: E402

W, H = 1920, 1080


def line(name, v, base=None):
    m = statistics.median(v)
    against = "" if base is None else f" = {m / statistics.median(base):.3f} x"
    return f"{name}: {m:.3f} ms{against}   {rounds(v)}"


def main():
    wl, r, st = c3_renderer(W, H)
    cam_a, cam_b = wl.scene.camera, moved(wl.scene.camera)
    base = wl.scene.node_array()

    # the node to move: seen from camera B
    frame_at(r, wl, st, cam_b)
    r.render_instance_plane(0, MISS_DEPTH)
    ids = r.read_instance_plane()
    count = np.bincount(ids[ids != capi.PT_INSTANCE_NONE].astype(np.int64), minlength=len(base))
    count[count >= 0.25 * W * H] = 0
    node = int(count.argmax())
    dist = float(np.linalg.norm(np.array(cam_a.center, np.float64) - np.array(cam_a.eye, np.float64)))
    after = base.copy()
    after[node]["worldMatrix"][12] += np.float32(0.02 * dist)
    print(f"{W}x{H}; {len(base)} nodes; node {node} moves by {0.02 * dist:.3f} along x and covers {100.0 * count[node] / (W * H):.1f} % of the image before the move")

    guides, inst7, inst0 = [], [], []
    for _ in range(ROUNDS):
        guides.append(stage_ms(r, "pt_debug_guides_time", 7, C.c_float(MISS_DEPTH)))
        inst7.append(stage_ms(r, "pt_debug_motion_time", None, 0, 7, C.c_float(MISS_DEPTH)))
        inst0.append(stage_ms(r, "pt_debug_motion_time", None, 0, 0, C.c_float(MISS_DEPTH)))
    table = {}
    found = {}
    for moments in (False, True):
        r.track_moments(moments)
        tag = "with moments" if moments else "no moments"
        for _ in range(ROUNDS):
            r.temporal_reset()
            r.update_instances(base)
            p_a = frame_at(r, wl, st, cam_a)
            r.render_instance_plane(7, MISS_DEPTH)
            r.temporal_accumulate_moving(p_a, read=False)
            r.update_instances(after)
            p_b = frame_at(r, wl, st, cam_b)
            r.render_instance_plane(7, MISS_DEPTH)
            table.setdefault(f"k_temporal, {tag}", []).append(stage_ms(r, "pt_debug_temporal_time", C.byref(p_b)))
            table.setdefault(f"k_temporal_moving, {tag}", []).append(stage_ms(r, "pt_debug_motion_time", C.byref(p_b), 1, 0, C.c_float(0.0)))
        on_node = r.read_instance_plane() == node
        r.temporal_accumulate_moving(p_b, read=False)
        _, length = r.read_temporal_history()
        found[tag] = (float((length[on_node] > 1).mean()), int(on_node.sum()))
    peaks = r.measure_peaks()
    copy_rate = peaks["hbmCopyBytesPerSec"]
    print(f"HBM float4 copy {copy_rate / 1e12:.2f} TB/s, read {peaks['hbmReadBytesPerSec'] / 1e12:.2f} TB/s (pt_measure_peaks, this run); 52 B per pixel = "
          f"{52 * W * H / copy_rate * 1e3:.3f} ms, 124 B per pixel = {124 * W * H / copy_rate * 1e3:.3f} ms, 140 B per pixel = {140 * W * H / copy_rate * 1e3:.3f} ms at the copy rate")
    print(line("k_guides, planes 7", guides))
    print(line("k_instances, planes 7", inst7, guides))
    print(line("k_instances, planes 0", inst0, guides))
    for moments in ("no moments", "with moments"):
        print(line(f"k_temporal, {moments}", table[f"k_temporal, {moments}"]))
        print(line(f"k_temporal_moving, {moments}", table[f"k_temporal_moving, {moments}"], table[f"k_temporal, {moments}"]))
    frac, n = found["no moments"]
    print(f"after the move {100.0 * frac:.1f} % of the {n} pixels of the moved node found history (length > 1) in the moving form")
    r.destroy()


if __name__ == "__main__":
    main()
