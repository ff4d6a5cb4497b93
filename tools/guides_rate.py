"""Time of the guide pass (pt_render_guides) on the Sponza stand-in (workloads C3) at 1920x1080, flat and two-level, against the composed route it
replaces and against the HBM streaming rate measured in the same run:

    python tools/guides_rate.py > profiles/guides_rate.txt          (--pass-only: (a) and (b) alone, for comparing builds of the library with PT_LIB)

(a) pt_render_guides(7) and (b) each single-plane mask, by device events (pt_debug_guides_time: the pass enqueued 50 times between two events after a
    warm-up run), the masks alternating over three rounds; the median is printed, the rounds next to it.
(c) the composed route, HipRenderer.render_guides: two frame-0 debug frames with pt_read_accum each, pixel-centre rays from numpy, pt_trace_rays on host
    arrays, three uploads through pt_set_denoise_guides -- host clock around the whole call, median of 10.
(d) for scale: one frame-0, 1 spp, maxDepth = 1 pt_render_frame with pt_synchronize, host clock, median of 10.
(e) pt_measure_peaks of the same run.  The traffic floor of the pass is one 48-byte write per pixel (the three planes) plus whatever the traversal and
    the hit's vertex, material and texture reads cost; the write alone is priced at the float4 copy rate.  A measurement, not a threshold."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rate_common import ROUNDS, HipRenderer, c3_workload, capi, hd, host_ms, rounds, stage_ms  # noqa: E402

W, H = 1920, 1080
MASKS = ((7, "all three planes"), (capi.PT_GUIDES_BASECOLOR, "base colour"), (capi.PT_GUIDES_NORMAL, "normal"), (capi.PT_GUIDES_DEPTH, "depth"))


def pass_ms(r, planes):
    return stage_ms(r, "pt_debug_guides_time", planes, 1.0e30)


def main():
    pass_only = "--pass-only" in sys.argv[1:]
    wl = c3_workload(W, H)
    # every prim-mesh of the stand-in is instantiated once: by default the two-level structure is the merged world-space one and the FLAT kernel
    # walks it; PT_TUNE mergeSingles=0 gives every prim-mesh its own object-space BLAS, which the two-level kernel walks
    for accel, tune, what in ((capi.PT_ACCEL_FLAT, None, "flat"), (capi.PT_ACCEL_TWO_LEVEL, None, "two-level (merged: flat kernel)"),
                              (capi.PT_ACCEL_TWO_LEVEL, "mergeSingles=0", "two-level, mergeSingles=0")):
        if tune is not None:
            os.environ["PT_TUNE"] = tune   # read by pt_create
        r = HipRenderer()
        r.setup(0)
        os.environ.pop("PT_TUNE", None)
        r.set_accel_mode(accel)
        r.set_scene(wl.scene)
        integral, _ = r.set_env(wl.env)
        r.set_camera(capi.camera_lookat(wl.scene.camera, W / H, nb_lights=len(wl.scene.lights)))
        r.set_sunsky(hd.default_sun_and_sky())
        r.create((W, H))
        table = {}
        for _ in range(ROUNDS):
            for planes, _name in MASKS:
                table.setdefault(planes, []).append(pass_ms(r, planes))
        for planes, name in MASKS:
            v = table[planes]
            print(f"{what}: pt_render_guides({planes}) {name}: {statistics.median(v):.3f} ms   {rounds(v)}")
        if pass_only:
            r.destroy()
            continue
        full = statistics.median(table[7])
        peaks = r.measure_peaks()
        copy_rate = peaks["hbmCopyBytesPerSec"]
        write_ms = 48.0 * W * H / copy_rate * 1e3
        print(f"{what}: HBM float4 copy {copy_rate / 1e12:.2f} TB/s, read {peaks['hbmReadBytesPerSec'] / 1e12:.2f} TB/s (pt_measure_peaks, this run); the {48 * W * H / 1e6:.0f} MB of "
              f"plane writes alone take {write_ms:.3f} ms at the copy rate: the pass takes {full / write_ms:.1f} times that (traversal, vertex, material and texture reads)")
        st = hd.default_rtx_state()
        st.size[0], st.size[1] = W, H
        st.maxDepth, st.pbrMode, st.fireflyClampThreshold = wl.depth, wl.pbr_mode, 4.0 * integral
        med, lo, hi = host_ms(lambda: r.render_guides(st))
        print(f"{what}: composed route (render_guides: 2 debug frames + 2 pt_read_accum + numpy rays + pt_trace_rays + pt_set_denoise_guides), host clock: "
              f"{med:.1f} ms (min {lo:.1f}, max {hi:.1f}); pt_render_guides(7) is {med / full:.0f} times faster")

        def guides_and_wait():
            r.capture_guides()
            r.synchronize()
        med, lo, hi = host_ms(guides_and_wait)
        print(f"{what}: pt_render_guides(7) + pt_synchronize, host clock: {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
        st.maxDepth, st.frame = 1, 0

        def one_frame():
            r.setPushContants(st)
            r.run()
            r.synchronize()
        med, lo, hi = host_ms(one_frame)
        print(f"{what}: one frame-0, 1 spp, maxDepth 1 pt_render_frame + pt_synchronize, host clock: {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
        r.destroy()


if __name__ == "__main__":
    main()
