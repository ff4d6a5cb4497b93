"""Time of what the responsive history adds to a call on the Sponza stand-in (workloads C3) at 1920x1080, after the camera move of
tools/temporal_rate.py:

    python tools/fast_rate.py > profiles/fast_rate.txt

The fast step (pt_debug_fast_time part 0) next to k_temporal of the same run (pt_debug_temporal_time with the setting off): it is the same kernel over
other pointers and should cost the same -- 120 B per pixel.  k_fast_clamp (part 1) for radius 1, 2 and 3 against its traffic floor of 60 B per pixel
(Hf' 16 + Hnf' 4 + Hc' 16 + Hn' 4 read, 20 written) at the HBM float4 copy rate pt_measure_peaks gives in the same run.  Device events (the kernel
enqueued 50 times between two events after a warm-up run of the whole call), three rounds in which the choices alternate, the median and the rounds
printed.  A measurement, not a threshold: no time is promised."""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rate_common import ROUNDS, c3_renderer, frame_at, moved, rounds, stage_ms  # noqa: E402

W, H = 1920, 1080
RADII = (1, 2, 3)


def line(name, v, base=None, floor_ms=None):
    m = statistics.median(v)
    against = "" if base is None else f" = {m / statistics.median(base):.3f} x"
    floor = "" if floor_ms is None else f"; {m / floor_ms:.2f} of its traffic floor of {floor_ms:.3f} ms"
    return f"{name}: {m:.3f} ms{against}{floor}   {rounds(v)}"


def main():
    wl, r, st = c3_renderer(W, H)
    cam_a, cam_b = wl.scene.camera, moved(wl.scene.camera)
    table = {}
    for _ in range(ROUNDS):
        for on in (False, True):
            r.temporal_fast(r.fast_params(4.0, 2.0, 2) if on else None)   # (drops the history: each choice is timed on a history of its own kind, made at camera A)
            p_a = frame_at(r, wl, st, cam_a)
            r.temporal_accumulate(p_a, read=False)
            p_b = frame_at(r, wl, st, cam_b)
            if not on:
                table.setdefault("k_temporal", []).append(stage_ms(r, "pt_debug_temporal_time", C.byref(p_b)))
                continue
            table.setdefault("fast step", []).append(stage_ms(r, "pt_debug_fast_time", C.byref(p_b), 0))
            for radius in RADII:
                r.temporal_fast(r.fast_params(4.0, 2.0, radius))          # (new parameters keep the history)
                table.setdefault(f"k_fast_clamp<{radius}>", []).append(stage_ms(r, "pt_debug_fast_time", C.byref(p_b), 1))
    r.temporal_fast(None)
    peaks = r.measure_peaks()
    copy_rate = peaks["hbmCopyBytesPerSec"]
    floor = lambda b: b * W * H / copy_rate * 1e3   # noqa: E731
    print(f"{W}x{H}; HBM float4 copy {copy_rate / 1e12:.2f} TB/s, read {peaks['hbmReadBytesPerSec'] / 1e12:.2f} TB/s (pt_measure_peaks, this run); 60 B per pixel = "
          f"{floor(60):.3f} ms, 120 B per pixel = {floor(120):.3f} ms at the copy rate")
    print(line("k_temporal (setting off)", table["k_temporal"], None, floor(120)))
    print(line("fast step (the same kernel over Hf, Hnf)", table["fast step"], table["k_temporal"], floor(120)))
    for radius in RADII:
        print(line(f"k_fast_clamp<{radius}>", table[f"k_fast_clamp<{radius}>"], None, floor(60)))
    r.destroy()


if __name__ == "__main__":
    main()
