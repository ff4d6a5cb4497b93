"""Time of the two kernels the demodulated history adds on the Sponza stand-in (workloads C3) at 1920x1080, each against what it
stands beside, timed in the same run:

    python tools/albedo_rate.py > profiles/albedo_rate.txt

k_temporal_d (pt_temporal_accumulate with pt_temporal_demodulate on) against k_temporal / k_temporal_m (the setting off) after the camera move of
tools/temporal_rate.py, with pt_temporal_track_moments off and on: it moves 16 B more per pixel than their 120 B (136 B with moments) -- the albedo load --
and does three divisions.  k_remodulate, the pass the consumers of a demodulated history append: 48 B per pixel (colour and albedo in, colour out).
Traffic floors at the HBM float4 copy rate of pt_measure_peaks in the same run are printed beside them.  Device events (pt_debug_temporal_time,
pt_debug_albedo_time: the kernel enqueued 50 times between two events after a warm-up run), three rounds in which the kernels alternate, the median and the
rounds printed.  A measurement, not a threshold: no time is promised."""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rate_common import ROUNDS, c3_renderer, frame_at, moved, rounds, stage_ms  # noqa: E402

W, H = 1920, 1080


def line(name, v, base=None, floor_ms=None):
    m = statistics.median(v)
    against = "" if base is None else f" = {m / statistics.median(base):.3f} x"
    floor = "" if floor_ms is None else f"; {m / floor_ms:.2f} of its traffic floor of {floor_ms:.3f} ms"
    return f"{name}: {m:.3f} ms{against}{floor}   {rounds(v)}"


def main():
    wl, r, st = c3_renderer(W, H)
    cam_a, cam_b = wl.scene.camera, moved(wl.scene.camera)
    table = {}
    for moments in (False, True):
        r.track_moments(moments)
        tag = "with moments" if moments else "no moments"
        for _ in range(ROUNDS):
            for on in (False, True):
                r.temporal_demodulate(on)            # (drops the history: each kernel is timed on a history of its own kind, made at camera A)
                p_a = frame_at(r, wl, st, cam_a)
                r.temporal_accumulate(p_a, read=False)
                p_b = frame_at(r, wl, st, cam_b)
                if on:
                    table.setdefault(f"k_temporal_d, {tag}", []).append(stage_ms(r, "pt_debug_albedo_time", C.byref(p_b), 0))
                else:
                    table.setdefault(f"k_temporal, {tag}", []).append(stage_ms(r, "pt_debug_temporal_time", C.byref(p_b)))
    remod = [stage_ms(r, "pt_debug_albedo_time", None, 1) for _ in range(ROUNDS)]
    peaks = r.measure_peaks()
    copy_rate = peaks["hbmCopyBytesPerSec"]
    floor = lambda b: b * W * H / copy_rate * 1e3   # noqa: E731
    print(f"{W}x{H}; HBM float4 copy {copy_rate / 1e12:.2f} TB/s, read {peaks['hbmReadBytesPerSec'] / 1e12:.2f} TB/s (pt_measure_peaks, this run); 16 B per pixel = "
          f"{floor(16):.3f} ms, 48 B per pixel = {floor(48):.3f} ms at the copy rate")
    for moments, bytes_px in (("no moments", 120), ("with moments", 136)):
        print(line(f"k_temporal{'_m' if bytes_px == 136 else ''}, {moments}", table[f"k_temporal, {moments}"], None, floor(bytes_px)))
        print(line(f"k_temporal_d, {moments}", table[f"k_temporal_d, {moments}"], table[f"k_temporal, {moments}"], floor(bytes_px + 16)))
    print(line("k_remodulate", remod, None, floor(48)))
    r.destroy()


if __name__ == "__main__":
    main()
