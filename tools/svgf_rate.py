"""Times of the variance-guided filter of the history on the Sponza stand-in (workloads C3) at 1920x1080 with three guide planes,
each against the k_denoise iteration of the same run and against its traffic floor at the HBM streaming rate measured in the same run:

    python tools/svgf_rate.py > profiles/svgf_rate.txt

Everything is timed with device events (pt_debug_temporal_time, pt_debug_svgf_time, pt_debug_denoise_time: the kernel enqueued 50 times between two events
after a warm-up run; no untile pass, no copy), three alternating rounds, the median and the rounds printed.

  k_temporal_m against k_temporal    after the tool's standard move (tools/temporal_rate.py's: a dolly, a strafe and a yaw), tracking on against tracking off
  k_svgf_variance                    its window staged in LDS (the default) and read from memory; the history all long (every pixel takes m2 - m1^2), all short
                                     (every pixel runs the 7 x 7 estimate) and after the standard move (four static calls, then the move: the disoccluded regions
                                     are short, the rest long)
  k_svgf<S> per iteration            steps 1 .. 16, in each form (S = 0 from memory, S = 1, 2 from LDS), against k_denoise<S> of the same step
  pt_measure_peaks                   the float4 copy rate

Traffic floor of a filter iteration: 68 B read (colour, three guide planes, variance) and 20 B written (colour, variance) per pixel = 182 MB; of k_denoise 64 + 16 =
166 MB.  The LDS default (SV_LDS_DEFAULT_STEP in csrc/pt_svgf.hip) is chosen from the ratios printed here.  A measurement, not a threshold."""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rate_common import ROUNDS, c3_renderer, frame_at, hd, med, moved, stage_ms  # noqa: E402

W, H, ITERATIONS = 1920, 1080, 5
SVGF_BYTES, DENOISE_BYTES = 88, 80
SIGMA_GUIDE = (1.0, 0.3, 0.5)


def main():
    wl, r, st = c3_renderer(W, H)
    L = r._lib

    def temporal_ms(p):
        return stage_ms(r, "pt_debug_temporal_time", C.byref(p))

    def svgf_ms(sp, what):
        return stage_ms(r, "pt_debug_svgf_time", C.byref(sp), what)

    def denoise_ms(n):
        return stage_ms(r, "pt_debug_denoise_time", C.byref(hd.DenoiseParams(iterations=n, sigmaColor=1.0, sigmaGuide=SIGMA_GUIDE, flags=0)))

    cam_a, cam_b = wl.scene.camera, moved(wl.scene.camera)
    t = {}

    def variance_ms(name, sp):
        """k_svgf_variance in both forms: the window staged in LDS (the default) and read from memory (pt_debug_svgf_lds 0)"""
        t.setdefault(name, []).append(svgf_ms(sp, -1))
        L.pt_debug_svgf_lds(r._ctx, 0)
        t.setdefault(name + " from memory", []).append(svgf_ms(sp, -1))
        L.pt_debug_svgf_lds(r._ctx, -1)

    long_share = 0.0
    for _ in range(ROUNDS):
        # the temporal kernel after the move, tracking off and on
        for on in (False, True):
            r.track_moments(on)
            r.temporal_accumulate(frame_at(r, wl, st, cam_a), read=False)
            t.setdefault("k_temporal_m" if on else "k_temporal", []).append(temporal_ms(frame_at(r, wl, st, cam_b)))
        # tracking is on: a first call (lengths 1), judged short by minTemporal 4 and long by minTemporal 1
        r.temporal_reset()
        p_a = frame_at(r, wl, st, cam_a)
        r.temporal_accumulate(p_a, read=False)
        variance_ms("variance short", r.svgf_params(ITERATIONS, sigma_guide=SIGMA_GUIDE, min_temporal=4.0))
        variance_ms("variance long", r.svgf_params(ITERATIONS, sigma_guide=SIGMA_GUIDE, min_temporal=1.0))
        for _ in range(3):
            r.temporal_accumulate(p_a, read=False)
        r.temporal_accumulate(frame_at(r, wl, st, cam_b), read=False)
        sp = r.svgf_params(ITERATIONS, sigma_guide=SIGMA_GUIDE, min_temporal=4.0)
        variance_ms("variance moved", sp)
        long_share = float((r.read_temporal_history()[1] >= 4.0).mean())
        for lds in (0, 1, 2):
            L.pt_debug_svgf_lds(r._ctx, lds)
            L.pt_debug_denoise_lds(r._ctx, lds)
            for i in range(ITERATIONS if lds == 0 else lds):
                t.setdefault(("svgf", lds, i), []).append(svgf_ms(sp, i))
            t.setdefault(("svgf whole", lds), []).append(svgf_ms(sp, -2))
            d = [0.0] + [denoise_ms(n) for n in range(1, (ITERATIONS if lds == 0 else lds) + 1)]
            for i in range(len(d) - 1):
                t.setdefault(("denoise", lds, i), []).append(d[i + 1] - d[i])
        L.pt_debug_svgf_lds(r._ctx, -1)
        L.pt_debug_denoise_lds(r._ctx, -1)
        t.setdefault("svgf default", []).append(svgf_ms(sp, -2))
        t.setdefault("denoise default", []).append(denoise_ms(ITERATIONS))
    peaks = r.measure_peaks()
    rate = peaks["hbmCopyBytesPerSec"]
    floor, dfloor = SVGF_BYTES * W * H / rate * 1e3, DENOISE_BYTES * W * H / rate * 1e3
    print(f"{W}x{H}, 3 guide planes, {ITERATIONS} iterations; HBM float4 copy {rate / 1e12:.2f} TB/s (pt_measure_peaks, this run); traffic floor of a filter iteration "
          f"{SVGF_BYTES} B per pixel = {SVGF_BYTES * W * H / 1e6:.0f} MB = {floor:.3f} ms, of a k_denoise iteration {DENOISE_BYTES * W * H / 1e6:.0f} MB = {dfloor:.3f} ms")
    a, b = statistics.median(t["k_temporal_m"]), statistics.median(t["k_temporal"])
    print(f"k_temporal_m after the move {med(t['k_temporal_m'])} against k_temporal {med(t['k_temporal'])}: {a / b:.2f} x")
    ref = statistics.median(t[("denoise", 2, 0)])
    for name, what in (("all long (minTemporal 1)", "variance long"), ("all short (minTemporal 4, lengths 1)", "variance short"),
                       (f"after the move ({100 * long_share:.1f} % of the pixels long)", "variance moved")):
        m = statistics.median(t[what])
        print(f"k_svgf_variance, {name}: {med(t[what])} = {m / ref:.2f} x a k_denoise<1> iteration; its window read from memory {med(t[what + ' from memory'])}")
    for lds in (0, 1, 2):
        for i in range(ITERATIONS if lds == 0 else lds):
            if lds and i != lds - 1:
                continue
            s, d = statistics.median(t[("svgf", lds, i)]), statistics.median(t[("denoise", lds, i)])
            print(f"k_svgf<{lds if lds else 0}> step {1 << i}: {med(t[('svgf', lds, i)])} = {s / floor:.1f} x its floor; k_denoise<{lds if lds else 0}> {d:.3f} ms = {d / dfloor:.1f} x its floor; ratio {s / d:.2f}")
    for lds in (0, 1, 2):
        print(f"LDS up to step {lds}: V0 and {ITERATIONS} iterations {med(t[('svgf whole', lds)])}")
    s, d = statistics.median(t["svgf default"]), statistics.median(t["denoise default"])
    print(f"default choice: V0 and {ITERATIONS} iterations {med(t['svgf default'])}; k_denoise, {ITERATIONS} iterations {d:.3f} ms; ratio {s / d:.2f}")
    r.destroy()


if __name__ == "__main__":
    main()
