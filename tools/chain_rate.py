"""Time of the chained guide pass (pt_render_guides_chain) on the Sponza stand-in (workloads C3) at 1920x1080, flat and two-level
(the second with PT_TUNE mergeSingles=0, so that the two-level kernel runs), against pt_render_guides of the same run:

    python tools/chain_rate.py > profiles/chain_rate.txt          (--pass-only: for comparing builds of the library with PT_LIB)

By device events (pt_debug_guides_chain_time / pt_debug_guides_time: the pass enqueued 50 times between two events after a warm-up run), the choices
alternating over three rounds; the median is printed, the rounds next to it.
(a) nothing followed: maxLinks = 8 with both classes off (minMetallic = minTransmission = 2) -- what the new kernel costs over pt_render_guides;
(b) everything followed: maxRoughness = 1, minMetallic = 0 at maxLinks 1, 2 and 4 -- the worst case, incoherent secondary walks on every pixel;
(c) the default thresholds (maxRoughness 0.05, minMetallic = minTransmission = 0.9) at maxLinks 4: what the stand-in's own materials make of it.
A measurement, not a threshold."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rate_common import ROUNDS, HipRenderer, c3_workload, capi, hd, rounds, stage_ms  # noqa: E402

W, H = 1920, 1080
MISS = 1.0e30


def chain(max_links, max_roughness, min_metallic, min_transmission):
    return hd.GuideChain(maxLinks=max_links, maxRoughness=max_roughness, minMetallic=min_metallic, minTransmission=min_transmission, flags=0)


CHOICES = (("pt_render_guides(7)", None),
           ("chain, nothing followed (maxLinks 8, both classes off)", chain(8, 1.0, 2.0, 2.0)),
           ("chain, everything followed, maxLinks 1", chain(1, 1.0, 0.0, 0.0)),
           ("chain, everything followed, maxLinks 2", chain(2, 1.0, 0.0, 0.0)),
           ("chain, everything followed, maxLinks 4", chain(4, 1.0, 0.0, 0.0)),
           ("chain, default thresholds, maxLinks 4", chain(4, 0.05, 0.9, 0.9)))


def main():
    import ctypes as C
    wl = c3_workload(W, H)
    for accel, tune, what in ((capi.PT_ACCEL_FLAT, None, "flat"), (capi.PT_ACCEL_TWO_LEVEL, "mergeSingles=0", "two-level, mergeSingles=0")):
        if tune is not None:
            os.environ["PT_TUNE"] = tune   # read by pt_create
        r = HipRenderer()
        r.setup(0)
        os.environ.pop("PT_TUNE", None)
        r.set_accel_mode(accel)
        r.set_scene(wl.scene)
        r.set_env(wl.env)
        r.set_camera(capi.camera_lookat(wl.scene.camera, W / H, nb_lights=len(wl.scene.lights)))
        r.set_sunsky(hd.default_sun_and_sky())
        r.create((W, H))
        table = {}
        for _ in range(ROUNDS):
            for name, p in CHOICES:
                ms = stage_ms(r, "pt_debug_guides_time", 7, MISS) if p is None else stage_ms(r, "pt_debug_guides_chain_time", C.byref(p), 7, MISS)
                table.setdefault(name, []).append(ms)
        for name, p in CHOICES:
            line = f"{what}: {name}: {statistics.median(table[name]):.3f} ms   {rounds(table[name])}"
            if p is not None:
                r.capture_guides_chain(p, 7, MISS)
                links = r.read_guide_chain()
                line += f"   links per pixel {float((links & 255).mean()):.3f}, pixels that follow any {float(((links & 255) > 0).mean()):.3f}"
            print(line)
        r.destroy()


if __name__ == "__main__":
    main()
