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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rate_common import ROUNDS, c3_renderer, frame_at, host_ms, moved, rounds, stage_ms  # noqa: E402

W, H = 1920, 1080
FLOOR_BYTES = 136    # per pixel: the floor the stage was specified against
KERNEL_BYTES = 120   # ... what k_temporal must move: 48 read (colour, normal, depth planes) + 36 read (history) + 36 written


def main():
    wl, r, st = c3_renderer(W, H)

    def temporal_ms(p):
        return stage_ms(r, "pt_debug_temporal_time", C.byref(p))

    cam_a, cam_b = wl.scene.camera, moved(wl.scene.camera)
    table = {}
    for _ in range(ROUNDS):
        r.temporal_reset()
        p_a = frame_at(r, wl, st, cam_a)
        table.setdefault("first call (no history)", []).append(temporal_ms(p_a))
        r.temporal_accumulate(p_a, read=False)
        p_b = frame_at(r, wl, st, cam_b)
        table.setdefault("after the camera move", []).append(temporal_ms(p_b))
        r.temporal_accumulate(p_b, read=False)
        _, length = r.read_temporal_history()
        table.setdefault("static camera", []).append(temporal_ms(p_b))
    peaks = r.measure_peaks()
    copy_rate = peaks["hbmCopyBytesPerSec"]
    floor_ms = FLOOR_BYTES * W * H / copy_rate * 1e3
    print(f"{W}x{H}; HBM float4 copy {copy_rate / 1e12:.2f} TB/s, read {peaks['hbmReadBytesPerSec'] / 1e12:.2f} TB/s (pt_measure_peaks, this run); traffic floor "
          f"{FLOOR_BYTES} B per pixel = {FLOOR_BYTES * W * H / 1e6:.0f} MB = {floor_ms:.3f} ms at the copy rate")
    print(f"after the move {100.0 * float((length > 1).mean()):.1f} % of the pixels found history (length > 1)")
    for name, v in table.items():
        med = statistics.median(v)
        print(f"k_temporal, {name}: {med:.3f} ms = {med / floor_ms:.2f} x the floor ({med / (floor_ms * KERNEL_BYTES / FLOOR_BYTES):.2f} x the {KERNEL_BYTES} B the kernel must move)   {rounds(v)}")
    a = host_ms(r.read_accum)
    b = host_ms(lambda: r.temporal_accumulate(p_b))
    c = host_ms(lambda: r.temporal_accumulate(p_b, read=False))
    print(f"host clock, synchronous calls: pt_read_accum {a[0]:.2f} ms, pt_temporal_accumulate with its image copied out {b[0]:.2f} ms (difference {b[0] - a[0]:.2f} ms), "
          f"without the copy {c[0]:.3f} ms (min {c[1]:.3f}, max {c[2]:.3f})")
    r.destroy()


if __name__ == "__main__":
    main()
