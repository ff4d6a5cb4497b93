"""pt_refit_accel against pt_build_accel on the same context, on the Sponza stand-in (workloads C3), flat and two-level, in one process:

    python tools/refit_rate.py > profiles/refit_rate.txt

The scene is deformed by a per-vertex displacement of about 1 % of the scene's extent and, for the record of what a caller must expect, about 20 % of it,
in two forms: a smooth wave (every component moved by amplitude x sin of the position along a diagonal, wavelength a quarter of the extent: neighbouring
vertices move together, as under skinning or cloth) and white noise (an independent normal offset per component: the worst case, neighbouring vertices
move apart and every small triangle becomes a large one -- for the rebuilt tree too).  Per mode and deformation: the host-clock time of
pt_update_vertices, of pt_refit_accel (its own pt_RefitInfo::ms) and of pt_build_accel from the same deformed vertices, medians of RUNS runs with the
runs listed; costAfter / costBefore of the refit that follows a build from the undeformed vertices; and the Msamples/s of a short frame sequence on the
refitted tree against the same sequence on a tree built from the deformed vertices (the images are bit-identical: tests/test_refit_gpu.py).
A measurement, not a threshold."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_common as rc  # noqa: E402
from rate_common import capi, hd, HipRenderer  # noqa: E402

W, H, RUNS, FRAMES = 1920, 1080, 7, 16


def ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def line(name, v):
    return f"  {name}: {statistics.median(v):.3f} ms {rc.rounds(v)}"


def frame_rate(r, st):
    """Msamples/s of FRAMES one-sample frames (frame 0 first), after one sequence that is not counted"""
    def seq():
        for f in range(FRAMES):
            st.frame = f
            r.setPushContants(st)
            r.run()
        r.synchronize()
    seq()
    out = []
    for _ in range(3):
        t, _ = ms(seq)
        out.append(W * H * FRAMES / (t * 1e-3) / 1e6)
    return out


def main():
    wl = rc.c3_workload(W, H)
    sc = wl.scene
    v0 = np.array(sc.vertices, copy=True)
    extent = float((v0["position"].max(0) - v0["position"].min(0)).max())
    print(f"{W}x{H}; {sc.num_triangles} triangles, {len(v0)} vertices, {len(sc.nodes)} nodes; extent of the vertex positions {extent:.3f}; medians of {RUNS} runs by the host clock")
    for accel, mode in ((capi.PT_ACCEL_FLAT, "flat"), (capi.PT_ACCEL_TWO_LEVEL, "two-level")):
        r = HipRenderer()
        r.setup(0)
        r.set_accel_mode(accel)
        r.set_scene(sc)
        integral, _ = r.set_env(wl.env)
        r.set_sunsky(hd.default_sun_and_sky())
        r.set_camera(capi.camera_lookat(sc.camera, W / H, nb_lights=len(sc.lights)))
        r.create((W, H))
        st = hd.default_rtx_state()
        st.size[0], st.size[1] = W, H
        st.maxDepth, st.pbrMode, st.fireflyClampThreshold = wl.depth, wl.pbr_mode, 4.0 * integral
        build = lambda: r._check(r._lib.pt_build_accel(r._ctx))
        print(f"== {mode}: Msamples/s on the tree as built from the undeformed vertices {statistics.median(frame_rate(r, st)):.1f}")
        for kind, frac in (("smooth wave", 0.01), ("smooth wave", 0.20), ("white noise", 0.01), ("white noise", 0.20)):
            v = v0.copy()
            if kind == "white noise":
                v["position"] += np.random.default_rng(int(frac * 100)).normal(0, frac * extent / np.sqrt(3.0), v["position"].shape).astype(np.float32)
            else:
                phase = 2.0 * np.pi * v0["position"].astype(np.float64).sum(1, keepdims=True) / (0.25 * extent) + np.array([0.0, 2.0, 4.0])
                v["position"] += (frac * extent / np.sqrt(3.0) * np.sin(phase)).astype(np.float32)
            # the cost ratio: a build from the undeformed vertices, then the deformation and one refit
            r.update_vertices(0, v0)
            build()
            r.update_vertices(0, v)
            first = r.refit_accel()
            t_update, t_refit, t_build = [], [], []
            for _ in range(RUNS):
                t_update.append(ms(lambda: r.update_vertices(0, v))[0])
                t_refit.append(r.refit_accel().ms)
            refit_rate = frame_rate(r, st)
            for _ in range(RUNS):
                r.update_vertices(0, v)
                t_build.append(ms(build)[0])
            built_rate = frame_rate(r, st)
            print(f"-- {kind}, displacement {100 * frac:.0f} % of the extent ({frac * extent:.3f}); {first.nodesWritten} nodes and {first.slotsWritten} leaf slots written; "
                  f"first refit after the build (makes the parent table) {first.ms:.3f} ms")
            print(line("pt_update_vertices (all vertices)", t_update))
            print(line("pt_refit_accel", t_refit))
            print(line("pt_build_accel", t_build))
            print(f"  refit / build = {statistics.median(t_refit) / statistics.median(t_build):.3f}")
            print(f"  costAfter / costBefore = {first.costAfter / first.costBefore:.3f}  ({first.costBefore:.6g} -> {first.costAfter:.6g})")
            a, b = statistics.median(refit_rate), statistics.median(built_rate)
            print(f"  Msamples/s, {FRAMES} frames of 1 spp: refitted tree {a:.1f} {rc.rounds(refit_rate)}, tree built from the deformed vertices {b:.1f} {rc.rounds(built_rate)}: refitted / built = {a / b:.3f}")
        r.destroy()


if __name__ == "__main__":
    main()
