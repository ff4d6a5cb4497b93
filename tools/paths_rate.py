"""Rate of pt_trace_paths against the frames of the same context, on the C3 stand-in at 1920x1080, depth 8:

    python tools/paths_rate.py > profiles/paths_rate.txt

The camera rays of frame 0 (tests/paths_host.py: camera_ray of pt_shade.h per pixel, with the seed after the camera's draws) are uploaded once and traced
in place (PT_RAYS_DEVICE) at 1 and at 4 samples per ray, on the flat and on the two-level structure: pt_debug_paths_time, device events around
rate_common.REPS launches after one untimed launch, in Mpaths/s (a path is one sample of one ray).  Next to it, from the same context: 20 profiled
frames of the workload, samples per second of the stage times pt_get_stats sums and by the host clock.  A frame runs the same paths staged, sorted into
queues and with a packet stage at bounce 0; the query carries each ray through all its bounces in one lane.  A measurement, not a threshold.

The device memory comes from the HIP runtime libptmi.so itself is linked against (ctypes on the library already in the process)."""
import ctypes as C
import time

import rate_common as rc
from rate_common import capi, hd, HipRenderer

from tests import paths_host  # noqa: E402  (rate_common has put the repository's root on the path)
from tests.common import Config  # noqa: E402

W, H, FRAMES = 1920, 1080, 20


def main():
    wl = rc.c3_workload(W, H)
    cfg = Config(wl.scene, wl.env, W, H, depth=wl.depth, pbr=wl.pbr_mode)
    ps = paths_host.PathScene(cfg)
    rays = ps.camera_rays(ps.state())
    ps.close()
    n = len(rays)
    hip = C.CDLL("libamdhip64.so.7")  # the runtime libptmi.so is linked against, already loaded
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    print(f"{n} camera rays of frame 0, depth {wl.depth}, traced in place on the device; device events around {rc.REPS} launches after 1 untimed")
    for accel, label in ((capi.PT_ACCEL_FLAT, "flat"), (capi.PT_ACCEL_TWO_LEVEL, "two-level")):
        r = HipRenderer()
        r.setup(0)
        r.set_accel_mode(accel)
        r.set_scene(wl.scene)
        integral, _ = r.set_env(wl.env)
        r.set_camera(cfg.camera)
        r.set_sunsky(hd.default_sun_and_sky())
        r.create((W, H))
        st = cfg.state(integral)
        d_rays, d_out = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_rays), rays.nbytes) == 0 and hip.hipMalloc(C.byref(d_out), n * 32) == 0
        assert hip.hipMemcpy(d_rays, rays.ctypes.data, rays.nbytes, 1) == 0
        for samples in (1, 4):
            st.maxSamples = samples
            ms = rc.stage_ms(r, "pt_debug_paths_time", C.byref(st), n, d_rays, d_out)
            print(f"{label:10s} pt_trace_paths, {samples} sample(s) per ray: {ms:9.3f} ms per launch   {n * samples / ms / 1e3:9.1f} Mpaths/s")
        hip.hipFree(d_rays); hip.hipFree(d_out)
        # the frames of the same context: 1 sample per pixel and frame
        st.maxSamples = 1
        for f in range(5):
            st.frame = f
            r.setPushContants(st); r.run()
        r.synchronize()
        r.set_profiling(1)
        r.reset_stats()
        t0 = time.perf_counter()
        for f in range(5, 5 + FRAMES):
            st.frame = f
            r.setPushContants(st); r.run()
        r.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        s = r.stats()
        stages = s["msGenerate"] + s["msTraceClosest"] + s["msShade"] + s["msTraceShadow"] + s["msAccumulate"] + s["msTail"] + s["msTraceFused"]
        print(f"{label:10s} frames, {FRAMES} profiled: {s['samples']} samples, stage times {stages:9.3f} ms -> {s['samples'] / max(stages, 1e-9) / 1e3:9.1f} Mpaths/s; "
              f"host clock {wall:9.3f} ms -> {s['samples'] / wall / 1e3:9.1f} Mpaths/s (the stage times add up kernels that overlap across the frames in flight)")
        r.destroy()


if __name__ == "__main__":
    main()
