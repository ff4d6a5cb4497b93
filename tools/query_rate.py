"""Rate of pt_trace_rays against the closest-hit stage of the frames, on the C3 stand-in at 1920x1080:

    python tools/query_rate.py > profiles/ray_query_rate.txt

The primary rays of the image (pinhole, one per pixel centre) are generated on the host, uploaded once, and traced in place (PT_RAYS_DEVICE) for each
kind: one warm-up call, five timed calls, the median in Mrays/s -- for the flat and for the two-level structure.  Next to each figure, from the same
process and context: the closest-hit stage's own rate, closestRays / msTraceClosest of pt_get_stats over a profiled 20-frame render.  The ratio says
what a query kernel on the persistent trace machine could gain ("Ray queries"); it is a measurement, not a threshold.

The device memory comes from the HIP runtime libptmi.so itself is linked against (ctypes on the library already in the process); renderer.py's
trace_rays_device takes any owner's addresses."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vk_raytrace_amd import capi, host_device as hd, workloads  # noqa: E402
from vk_raytrace_amd.renderer import HipRenderer  # noqa: E402

KINDS = (("CLOSEST", capi.PT_RAYS_CLOSEST, 1), ("OCCLUDED", capi.PT_RAYS_OCCLUDED, 1), ("NEAREST", capi.PT_RAYS_NEAREST, 1), ("CANDIDATES x4", capi.PT_RAYS_CANDIDATES, 4))


def primary_rays(cam, width, height):
    """camera rays through the pixel centres (pinhole): the formula of tests/host_harness.py deep_rays"""
    t = np.tan(np.radians(cam.fov) / 2)
    ys, xs = np.mgrid[0:height, 0:width]
    d = np.stack([(2 * (xs + 0.5) / width - 1) * t * width / height, (1 - 2 * (ys + 0.5) / height) * t, np.ones(xs.shape)], -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(len(d), hd.ray_dtype)
    rays["origin"], rays["direction"] = np.asarray(cam.eye, np.float32), d.astype(np.float32)
    rays["tmax"] = np.inf
    rays["seed"] = np.arange(len(d), dtype=np.uint32) * np.uint32(2654435761)
    return rays


def main():
    wl = workloads.c3_sponza()
    if wl.scene.vertices is None:
        wl.scene.finalize(capi.pack_vertices)
    rays = primary_rays(wl.scene.camera, wl.width, wl.height)
    n = len(rays)
    capi.lib()
    hip = C.CDLL("libamdhip64.so.7")  # the runtime libptmi.so is linked against, already loaded
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    print(f"{wl.name}: {n} primary rays, traced in place on the device; median of 5 calls after 1 warm-up")
    for accel, label in ((capi.PT_ACCEL_FLAT, "flat"), (capi.PT_ACCEL_TWO_LEVEL, "two-level")):
        r = HipRenderer()
        r.setup(0)
        r.set_accel_mode(accel)
        r.set_scene(wl.scene)
        integral, _ = r.set_env(wl.env)
        r.set_camera(capi.camera_lookat(wl.scene.camera, wl.width / wl.height, nb_lights=len(wl.scene.lights)))
        r.set_sunsky(hd.default_sun_and_sky())
        r.create((wl.width, wl.height))
        d_rays, d_hits = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_rays), rays.nbytes) == 0 and hip.hipMalloc(C.byref(d_hits), n * 4 * 32) == 0
        assert hip.hipMemcpy(d_rays, rays.ctypes.data, rays.nbytes, 1) == 0
        rates = {}
        for name, kind, hpr in KINDS:
            r.trace_rays_device(kind, d_rays.value, d_hits.value, n, hpr)
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                r.trace_rays_device(kind, d_rays.value, d_hits.value, n, hpr)
                ts.append(time.perf_counter() - t0)
            rates[name] = n / statistics.median(ts) / 1e6
        hip.hipFree(d_rays); hip.hipFree(d_hits)
        # the closest-hit stage of the frames: 20 profiled frames of the workload
        st = hd.default_rtx_state()
        st.size[0], st.size[1] = wl.width, wl.height
        st.maxDepth, st.pbrMode, st.fireflyClampThreshold = wl.depth, wl.pbr_mode, 4.0 * integral
        for f in range(5):
            st.frame = f
            r.setPushContants(st); r.run()
        r.synchronize()
        r.set_profiling(1)
        r.reset_stats()
        for f in range(5, 25):
            st.frame = f
            r.setPushContants(st); r.run()
        r.synchronize()
        s = r.stats()
        stage = s["closestRays"] / max(s["msTraceClosest"] + s["msTraceFused"] + s["msTail"], 1e-9) / 1e3
        stage0 = s["closestRays"] / max(s["msTraceClosest"], 1e-9) / 1e3
        for name, _, _ in KINDS:
            print(f"{label:10s} {name:14s} {rates[name]:9.1f} Mrays/s   closest stage, 20 profiled frames: closestRays / msTraceClosest = {stage0:9.1f} Mrays/s   ratio {rates[name] / stage0:5.2f}")
        print(f"{label:10s} (closestRays {s['closestRays']}, msTraceClosest {s['msTraceClosest']:.2f}, msTraceFused {s['msTraceFused']:.2f}, msTail {s['msTail']:.2f}: "
              f"closestRays over all three = {stage:.1f} Mrays/s, a lower bound -- the fused stage and the tail also trace shadow rays and shade)")
        r.destroy()


if __name__ == "__main__":
    main()
