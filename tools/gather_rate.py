"""Rate of pt_gather against pt_trace_paths in the same context, on the C3 stand-in, depth 8:

    python tools/gather_rate.py > profiles/gather_rate.txt

2^18 points on the scene's surfaces (random triangles, random barycentrics, the triangle's normal turned towards the side the camera is on) are uploaded
once and gathered in place (PT_RAYS_DEVICE) at 16 and at 64 samples per point, both kinds, on the flat and on the two-level structure:
pt_debug_gather_time, device events around rate_common.REPS launches after one untimed launch, in Mpaths/s (a path is one sample of one point).  Next to
it, in the same context, pt_debug_paths_time on the same number of one-sample camera rays (frame 0's, repeated with other seeds): coherent first
bounces against the gather's incoherent ones.  Last, by the host clock on the flat structure at 16 samples: pt_gather on host arrays, and the route it
replaces -- points x samples rays made with numpy, pt_trace_paths on host arrays, a numpy reduction.  A measurement, not a threshold.

The device memory comes from the HIP runtime libptmi.so itself is linked against (ctypes on the library already in the process)."""
import ctypes as C
import time

import numpy as np

import rate_common as rc
from rate_common import capi, hd, HipRenderer

from tests import paths_host  # noqa: E402  (rate_common has put the repository's root on the path)
from tests.common import Config  # noqa: E402

W, H, POINTS = 1920, 1080, 1 << 18
KINDS = ((capi.PT_GATHER_HEMISPHERE, "hemisphere", 32), (capi.PT_GATHER_SPHERE, "sphere", 128))


def surface_points(scene, n, rng):
    """n points on the scene's triangles, area-blind: (positions, unit normals towards the camera's side), float32"""
    pos, idx = np.asarray(scene.vertices["position"], np.float64), np.asarray(scene.indices, np.int64)
    tris = []
    for m, pm in scene.nodes:
        vo, vc, fi, ic, _ = scene.prim_meshes[pm]
        if ic >= 3:
            m = np.asarray(m, np.float64)
            tris.append((pos[vo + idx[fi:fi + ic]] @ m[:3, :3].T + m[:3, 3]).reshape(-1, 3, 3))
    tris = np.concatenate(tris)
    t = tris[rng.integers(0, len(tris), n)]
    b = rng.dirichlet((1, 1, 1), n)
    p = (t * b[:, :, None]).sum(1)
    g = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    g /= np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-30)
    g[np.linalg.norm(g, axis=1) < 0.5] = (0, 1, 0)
    eye = np.asarray(scene.camera.eye, np.float64)
    g *= np.where(((eye - p) * g).sum(1) < 0, -1.0, 1.0)[:, None]
    return p.astype(np.float32), g.astype(np.float32)


def numpy_cosine_rays(points, samples, rng):
    """what a baker does without pt_gather: points x samples cosine-distributed rays about the normals, with numpy's generator and numpy's sin / cos"""
    n = len(points)
    N = points["normal"].astype(np.float32)
    a = np.where(np.abs(N[:, :1]) > 0.9, np.float32([0, 1, 0]), np.float32([1, 0, 0]))
    T = np.cross(a, N); T /= np.linalg.norm(T, axis=1, keepdims=True)
    B = np.cross(N, T)
    r1, r2 = rng.random((n, samples), np.float32), rng.random((n, samples), np.float32)
    r, phi = np.sqrt(r1), np.float32(2 * np.pi) * r2
    x, y, z = r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(0, 1 - r1))
    rays = np.zeros((n, samples), hd.ray_dtype)
    rays["origin"] = (points["position"] + np.float32(1e-4) * N)[:, None, :]
    rays["direction"] = x[..., None] * T[:, None, :] + y[..., None] * B[:, None, :] + z[..., None] * N[:, None, :]
    rays["tmax"] = np.inf
    rays["seed"] = rng.integers(0, 2 ** 32, (n, samples), dtype=np.uint64).astype(np.uint32)
    return rays


def main():
    wl = rc.c3_workload(W, H)
    cfg = Config(wl.scene, wl.env, W, H, depth=wl.depth, pbr=wl.pbr_mode)
    ps = paths_host.PathScene(cfg)
    cam_rays = ps.camera_rays(ps.state())
    ps.close()
    rng = np.random.default_rng(2718)
    p, nrm = surface_points(wl.scene, POINTS, rng)
    pts = np.zeros(POINTS, hd.gatherpoint_dtype)
    pts["position"], pts["normal"], pts["seed"] = p, nrm, rng.integers(0, 2 ** 32, POINTS, dtype=np.uint64).astype(np.uint32)
    hip = C.CDLL("libamdhip64.so.7")  # the runtime libptmi.so is linked against, already loaded
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    print(f"{POINTS} points on the scene's surfaces, depth {wl.depth}, gathered in place on the device; device events around {rc.REPS} launches after 1 untimed")
    for accel, label in ((capi.PT_ACCEL_FLAT, "flat"), (capi.PT_ACCEL_TWO_LEVEL, "two-level")):
        r = HipRenderer()
        r.setup(0)
        r.set_accel_mode(accel)
        r.set_scene(wl.scene)
        integral, _ = r.set_env(wl.env)
        r.set_camera(cfg.camera)
        r.set_sunsky(hd.default_sun_and_sky())
        st = cfg.state(integral)
        d_pts, d_out = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_pts), pts.nbytes) == 0 and hip.hipMalloc(C.byref(d_out), POINTS * 128) == 0
        assert hip.hipMemcpy(d_pts, pts.ctypes.data, pts.nbytes, 1) == 0
        for samples in (16, 64):
            st.maxSamples = samples
            for kind, name, _ in KINDS:
                ms = rc.stage_ms(r, "pt_debug_gather_time", C.byref(st), kind, POINTS, d_pts, d_out)
                print(f"{label:10s} pt_gather {name:10s} {samples:3d} samples per point: {ms:9.3f} ms per launch   {POINTS * samples / ms / 1e3:9.1f} Mpaths/s")
            # the same number of one-sample camera rays through pt_trace_paths
            n = POINTS * samples
            rays = np.resize(cam_rays, n)
            rays["seed"] = rays["seed"] + (np.arange(n, dtype=np.uint64) // np.uint64(len(cam_rays))).astype(np.uint32) * np.uint32(2654435761)
            d_rays, d_res = C.c_void_p(), C.c_void_p()
            assert hip.hipMalloc(C.byref(d_rays), rays.nbytes) == 0 and hip.hipMalloc(C.byref(d_res), n * 32) == 0
            assert hip.hipMemcpy(d_rays, rays.ctypes.data, rays.nbytes, 1) == 0
            st.maxSamples = 1
            ms = rc.stage_ms(r, "pt_debug_paths_time", C.byref(st), n, d_rays, d_res)
            print(f"{label:10s} pt_trace_paths, {n} one-sample camera rays:   {ms:9.3f} ms per launch   {n / ms / 1e3:9.1f} Mpaths/s")
            hip.hipFree(d_rays); hip.hipFree(d_res)
            del rays
        hip.hipFree(d_pts); hip.hipFree(d_out)
        if accel == capi.PT_ACCEL_FLAT:
            # host arrays, host clock, 16 samples: the call, and the route it replaces
            samples = 16
            st.maxSamples = samples
            t0 = time.perf_counter()
            got = r.gather_records(st, capi.PT_GATHER_HEMISPHERE, pts)
            t_gather = (time.perf_counter() - t0) * 1e3
            one = hd.RtxState.from_buffer_copy(st); one.maxSamples = 1
            t0 = time.perf_counter()
            rays = numpy_cosine_rays(pts, samples, np.random.default_rng(1))
            t_make = (time.perf_counter() - t0) * 1e3
            rec = r.trace_path_records(one, rays.reshape(-1))
            t_trace = (time.perf_counter() - t0) * 1e3 - t_make
            irr = rec["radiance"].reshape(POINTS, samples, 3).sum(1) * np.float32(np.pi / samples)
            t_all = (time.perf_counter() - t0) * 1e3
            print(f"{label:10s} host arrays, hemisphere, {samples} samples, host clock: pt_gather {t_gather:9.1f} ms; the host route {t_all:9.1f} ms "
                  f"(numpy rays {t_make:.1f} + pt_trace_paths {t_trace:.1f} + numpy reduction {t_all - t_make - t_trace:.1f}) -> {t_all / t_gather:.1f} x; "
                  f"mean irradiance {got['irradiance'].mean():.4f} against {irr.mean():.4f}")
        r.destroy()


if __name__ == "__main__":
    main()
