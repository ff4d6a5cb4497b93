"""Time of the denoiser at 1920x1080 with three guide planes and 5 iterations, against the HBM streaming rate measured in the same run:

    python tools/denoise_rate.py > profiles/denoise_rate.txt

The filter alone is timed with device events (pt_debug_denoise_time: the kernels of pt_denoise enqueued 50 times between two events after a warm-up run; no
untile pass, no copy), for every choice of which steps stage their tile in LDS (pt_debug_denoise_lds 0, 1, 2), the choices alternating over three rounds; the
median of the rounds is printed.  Iteration counts 1 and 2 isolate steps 1 and 2, the only ones the choice changes.  The host-side cost of the synchronous
entry points is reported separately: pt_denoise against pt_read_accum (both end in the copy of the 33 MB image to pageable host memory), median of 10 calls.

Fraction of the streaming rate: the least traffic of an iteration is one read of the colour image and of each guide plane plus one write of the colour
image, 16 bytes per pixel each, over the iteration's share of the measured time, against pt_measure_peaks' float4 copy rate (read + written bytes per
second).  It is a measurement, not a threshold."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rate_common import ROUNDS, HipRenderer, capi, hd, rounds, stage_ms  # noqa: E402

W, H, ITERATIONS = 1920, 1080, 5


def inputs(rng):
    """a noisy image over smooth guides with edges: the filter's time does not depend on the values beyond which taps are finite"""
    ys, xs = np.mgrid[0:H, 0:W]
    colour = np.ones((H, W, 4), np.float32)
    colour[..., :3] = rng.gamma(0.5, 2.0, (H, W, 3)).astype(np.float32)
    albedo = np.zeros((H, W, 4), np.float32)
    albedo[..., :3] = np.where(((xs // 240 + ys // 270) % 2 == 0)[..., None], (0.8, 0.6, 0.4), (0.2, 0.3, 0.9))
    normal = np.zeros((H, W, 4), np.float32)
    normal[..., 0], normal[..., 1] = np.sin(xs / 200.0), np.cos(ys / 150.0)
    depth = np.zeros((H, W, 4), np.float32)
    depth[..., 0] = 2.0 + ys / H * 10.0 + (xs // 480)
    return colour, (albedo, normal, depth)


def filter_ms(r, p):
    return stage_ms(r, "pt_debug_denoise_time", C.byref(p))


def main():
    r = HipRenderer()
    r.setup(0)
    r.create((W, H))
    colour, guides = inputs(np.random.default_rng(1))
    r.write_accum(colour)
    r.set_denoise_guides(*guides)
    peaks = r.measure_peaks()
    copy_rate = peaks["hbmCopyBytesPerSec"]
    print(f"{W}x{H}, 3 guide planes; HBM float4 copy {copy_rate / 1e12:.2f} TB/s, read {peaks['hbmReadBytesPerSec'] / 1e12:.2f} TB/s (pt_measure_peaks, this run)")
    min_bytes = (2 + capi.PT_DENOISE_GUIDES) * 16 * W * H
    table = {}
    for _ in range(ROUNDS):
        for lds in (0, 1, 2):
            assert capi.lib().pt_debug_denoise_lds(r._ctx, lds) == lds
            for its, flags in ((1, 0), (2, 0), (ITERATIONS, 0), (ITERATIONS, capi.PT_DENOISE_DEMODULATE)):
                p = hd.DenoiseParams(iterations=its, sigmaColor=1.0, sigmaGuide=(0.1, 0.3, 0.5), flags=flags)
                table.setdefault((lds, its, flags), []).append(filter_ms(r, p))
    med = {k: statistics.median(v) for k, v in table.items()}
    for lds in (0, 1, 2):
        s1, s2, full, dem = med[(lds, 1, 0)], med[(lds, 2, 0)] - med[(lds, 1, 0)], med[(lds, ITERATIONS, 0)], med[(lds, ITERATIONS, 1)]
        print(f"LDS up to step {lds}: step 1 {s1:.3f} ms, step 2 {s2:.3f} ms, {ITERATIONS} iterations {full:.3f} ms ({full / ITERATIONS:.3f} ms each, "
              f"{min_bytes / (full / ITERATIONS * 1e-3) / copy_rate:.3f} of the copy rate at {min_bytes / 1e6:.0f} MB least traffic each), with demodulation {dem:.3f} ms"
              f"   {rounds(table[(lds, ITERATIONS, 0)])}")
    capi.lib().pt_debug_denoise_lds(r._ctx, -1)
    p = hd.DenoiseParams(iterations=ITERATIONS, sigmaColor=1.0, sigmaGuide=(0.1, 0.3, 0.5), flags=0)
    print(f"default choice: {ITERATIONS} iterations {filter_ms(r, p):.3f} ms")
    host = {"pt_read_accum": [], "pt_denoise": []}
    r.read_accum(), r.denoise(p)
    for _ in range(10):
        for name, fn in (("pt_read_accum", r.read_accum), ("pt_denoise", lambda: r.denoise(p))):
            t0 = time.perf_counter()
            fn()
            host[name].append((time.perf_counter() - t0) * 1e3)
    a, b = statistics.median(host["pt_read_accum"]), statistics.median(host["pt_denoise"])
    print(f"host clock, synchronous calls with the copy of the image to host memory: pt_read_accum {a:.2f} ms, pt_denoise {b:.2f} ms (difference {b - a:.2f} ms)")
    r.destroy()


if __name__ == "__main__":
    main()
