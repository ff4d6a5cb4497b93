"""Shared by tests/test_path_model.py, tests/test_path_gpu.py and tests/golden/measure_path_kat.py: the fixture of tests/golden/gen_path_kat.py, the scene and
the configurations it describes, and every leg's whole-frame entry on them.  A leg is a function (cfg, frames) -> accumulation image."""
import importlib.util
import json
import os

import numpy as np

from tests import surface_kat_io
from vk_raytrace_amd import host_device as hd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 4.0


def generator():
    spec = importlib.util.spec_from_file_location("gen_path_kat", os.path.join(GOLDEN, "gen_path_kat.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def load(path=None):
    """the fixture: path_kat.npz and path_kat_sky.npz as one (image_names and config_names list both), with the environment and its recorded alias table
    (path_kat_env.npz: env, env_table, env_integral, env_average)"""
    out = {}
    path = path or os.path.join(GOLDEN, "path_kat.npz")
    for p in (os.path.join(GOLDEN, "path_kat_env.npz"), path, path[:-4] + "_sky.npz"):   # (_sky: the images of the sun & sky configurations, and the SunAndSky words)
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    out["image_names"] = np.concatenate([out["image_names"], out["sky_image_names"]])
    out["config_names"] = np.concatenate([out["config_names"], out["sky_config_names"]])
    return out


def tolerances():
    with open(os.path.join(GOLDEN, "path_kat_tol.json")) as f:
        return json.load(f)["images"]


def fixture_scene(kat, nb_lights):
    """the fixture's arrays as a Scene with the first nb_lights lights (the vertices word for word, one prim-mesh record and one identity node per piece)"""
    sc = surface_kat_io.fixture_scene(kat)
    assert kat["lights"].dtype.itemsize == hd.light_dtype.itemsize
    sc.lights = list(np.frombuffer(kat["lights"].tobytes(), hd.light_dtype).copy())[:nb_lights]
    return sc


def config(kat, name, debug=0, depth=None):
    """tests.common.Config of a fixture configuration; the camera words are the fixture's, not pt_camera_lookat's"""
    from tests.common import Config
    nb, hdr, pbr, cdepth, aperture, ms, variant, firefly = (float(x) for x in kat["cfg_" + name])
    w, h = (int(x) for x in kat["size"])
    if name in kat["sky_config_names"]:   # sun & sky in use: the fixture's words, to every leg
        sun = hd.SunAndSky.from_buffer_copy(np.ascontiguousarray(kat["sunsky"], np.float32).tobytes())
        assert sun.in_use == 1
    else:
        sun = hd.default_sun_and_sky()
        sun.in_use = 0
    cfg = Config(fixture_scene(kat, int(nb)), kat["env"], w, h, depth=int(cdepth) if depth is None else depth, pbr=int(pbr), sunsky=sun, debug=debug,
                 max_samples=int(ms), hdr_multiplier=hdr, firefly=firefly, variant=int(variant))
    cam = hd.SceneCamera()
    cam.viewInverse[:], cam.projInverse[:] = [float(x) for x in kat["viewInverse"]], [float(x) for x in kat["projInverse"]]
    cam.focalDist, cam.aperture, cam.nbLights = float(kat["focalDist"]), aperture, int(nb)
    cfg.camera = cam
    return cfg


def parse(name):
    """image name -> (configuration, frames, debug mode, depth or None)"""
    gen_modes = {"radiance": hd.eRadiance, "weight": hd.eWeight, "raydir": hd.eRayDir}
    cn, what = name.rsplit("_", 1)
    if what.startswith("acc"):
        return cn, int(what[3:]), 0, None
    mode = what.rstrip("0123456789")
    return cn, 1, gen_modes[mode], int(what[len(mode):])


def render_all(kat, leg):
    """every image of the fixture through one leg -> (name, (H, W, 4) float32) pairs.  Every entry renders from frame 0: acc1, acc2 and acc3 of a configuration are
    three runs of 1, 2 and 3 frames."""
    for name in kat["image_names"]:
        cn, frames, debug, depth = parse(str(name))
        yield str(name), leg(config(kat, cn, debug, depth), frames)


def error(kat, name, img):
    """-> (max over the kept pixels of |got - f64| / max(1, |f64|), number of kept pixels); a non-finite value on a kept pixel is an infinite error"""
    kept, want = kat["kept_" + name], kat["img_" + name]
    got = img[..., :3].astype(np.float64)[kept]
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want[kept]) / np.maximum(1.0, np.abs(want[kept]))
    e[~np.isfinite(e)] = np.inf
    return (float(e.max()) if e.size else 0.0), int(kept.sum())


def check(kat, tol, name, img):
    """the bound of the model tests: 4 x the reference's recorded maximum, equality where that is 0"""
    e, _ = error(kat, name, img)
    bound = FACTOR * tol[name]["max"]
    print(f"{name:18s} error {e:.3e} bound {bound:.3e}")
    assert e <= bound, f"{name}: {e:.3e} against the model exceeds {bound:.3e}"


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- legs --------------------------------------------------------------------------------------------------------------------------------------------------
def oracle(cfg, frames):
    from tests.common import render_oracle
    return render_oracle(cfg, frames)


def reference(cfg, frames):
    from tests.ref import render_reference
    return render_reference(cfg, frames)


def host(two):
    def leg(cfg, frames):
        from tests.host_harness import host_render
        return host_render(cfg, frames, two=two)
    return leg


def device_images(kat, accel, tune=None):
    """every image of the fixture from the device -> ({name: image}, {configuration: bounces its third frame ran staged}).  One HipRenderer per configuration (PT_TUNE = tune while it is created: pt_create reads it):
    the accumulation image is read after each of the three frames, then the debug images are single frames with frame = 0, which replace the buffer."""
    from vk_raytrace_amd import capi
    from vk_raytrace_amd.renderer import HipRenderer
    out, staged = {}, {}
    keep = os.environ.get("PT_TUNE")
    for cn in kat["config_names"]:
        cn = str(cn)
        cfg = config(kat, cn)
        if tune is not None:
            os.environ["PT_TUNE"] = tune
        try:
            r = HipRenderer()
            r.setup(0)
        finally:
            if tune is not None:
                if keep is None:
                    del os.environ["PT_TUNE"]
                else:
                    os.environ["PT_TUNE"] = keep
        try:
            r.set_accel_mode(accel)
            r.set_scene(cfg.scene)
            integral, _ = r.set_env(cfg.env)
            r.set_camera(cfg.camera)
            r.set_sunsky(cfg.sunsky)
            r.set_variant(cfg.variant)
            r.useAnyHit(cfg.any_hit)
            r.create((cfg.width, cfg.height))
            for name in kat["image_names"]:
                name = str(name)
                c2, frames, debug, depth = parse(name)
                if c2 != cn:
                    continue
                st = config(kat, cn, debug, depth).state(integral)
                st.frame = frames - 1 if debug == 0 else 0   # (image_names lists acc1, acc2, acc3 in order)
                r.setPushContants(st)
                r.run(None, (cfg.width, cfg.height), None, None)
                out[name] = r.read_accum()
                # the route the launch sequence took (pt_debug.hip): the bounces before k_tail took over, that bounce included.  Read once per configuration, after
                # the third accumulation frame: the debug frames run in the same context under the same policy, their route is not read again
                if debug == 0 and frames == 3:
                    counts = np.zeros((16, 16), np.uint32)
                    staged[cn] = capi.lib().pt_debug_bounce_counts(r._ctx, counts.ctypes.data, 16)
        finally:
            r.destroy()
    return out, staged
