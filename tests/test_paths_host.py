"""pt_trace_paths' per-ray body on the CPU: vk_raytrace_amd/csrc/pt_paths.h (path_query<TWO>, what the path-query kernel runs per lane) compiled for the
host by tests/cpp/paths_host.cpp (tests/paths_host.py) and held to DESIGN.md section 3.2 -- to the oracle's frames bit for bit (anchors 1 and 2), to
itself (composition) and to the edges the definition names.  tests/test_paths_gpu.py runs the same rays through the C ABI on the device and compares
them, record by record, with what this build returns (the helpers below are shared with it)."""
import functools
import shutil
import subprocess

import numpy as np
import pytest

from tests import paths_host
from tests.common import Config, render_oracle
from tests.test_query_host import DEGENERATE_DIR, DEGENERATE_ORG, bits, empty_scenes, invalid_ray_cases, make_rays, one_triangle_scene, records_equal
from vk_raytrace_amd import capi, host_device as hd, synth

HIT, INVALID = capi.PT_RAY_HIT, capi.PT_RAY_INVALID
LUMA = np.array([0.212671, 0.715160, 0.072169], np.float32)


@functools.lru_cache(None)
def sky():
    return synth.procedural_sky(128, 64)


def config(name, max_samples=1, aperture=None):
    """the configurations of the whole-frame host test (tests/test_trace_host.py), frame 0"""
    if name in ("feature box disney", "feature box gltf"):
        return Config(synth.feature_box(tex_size=32, lights=True), sky(), 64, 48, depth=6, pbr=int(name.endswith("gltf")), max_samples=max_samples)
    if name == "fuzz 2 rtx sun & sky":
        ss = hd.default_sun_and_sky(); ss.in_use = 1
        return Config(synth.fuzz_scene(2), sky(), 96, 64, depth=5, variant=capi.PT_VARIANT_RTX, sunsky=ss, max_samples=max_samples)
    if name == "fuzz 4 depth of field":
        sc = synth.fuzz_scene(4); sc.camera.aperture = 0.05 if aperture is None else aperture
        return Config(sc, sky(), 50, 37, depth=4, hdr_multiplier=2.0, max_samples=max_samples)
    if name == "normal aov":
        return Config(synth.feature_box(tex_size=32), sky(), 64, 48, debug=hd.eNormal)
    if name == "depth 0":
        return Config(synth.feature_box(tex_size=32, lights=True), sky(), 64, 48, depth=0)
    raise KeyError(name)


ANCHOR_1 = ["feature box disney", "feature box gltf", "fuzz 2 rtx sun & sky", "fuzz 4 depth of field", "normal aov", "depth 0"]


@functools.lru_cache(None)
def oracle_frame0(name, max_samples=1):
    return render_oracle(config(name, max_samples), 1)


def same_pixels(got, want):
    """bit for bit, except that a NaN may match any NaN (and only a NaN)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def luma(rgb):
    """dot3(r, luminance weights) in fp32, in the order the clamp evaluates it"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    return (rgb[..., 0] * LUMA[0] + rgb[..., 1] * LUMA[1]) + rgb[..., 2] * LUMA[2]


def image(cfg, records):
    return records["radiance"].reshape(cfg.height, cfg.width, 3)


def chained(ps, two, st, rays, samples, skip):
    """`samples` one-sample calls on the same rays, each continuing from the previous call's seed advanced by `skip` draws: the records of every call"""
    one = hd.RtxState.from_buffer_copy(st)
    one.maxSamples = 1
    rays, out = rays.copy(), []
    for s in range(samples):
        out.append(ps.paths(two, one, rays))
        rays["seed"] = paths_host.advance(out[-1]["seed"], skip)
    return out


def mean_of(calls):
    total = np.zeros_like(calls[0]["radiance"])
    for c in calls:
        total = total + c["radiance"]   # fp32, in sample order
    return total / np.float32(len(calls))


# ---- anchor 1: one sample on the camera rays of frame 0 is frame 0 ------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [0, 1], ids=["flat", "two-level"])
@pytest.mark.parametrize("name", ANCHOR_1)
def test_one_sample_on_the_camera_rays_is_the_oracles_frame(name, two):
    cfg = config(name)
    ps = paths_host.PathScene(cfg)
    st = ps.state()
    rays = ps.camera_rays(st)
    got = ps.paths(two, st, rays)
    want = oracle_frame0(name)[..., :3]
    same = same_pixels(image(cfg, got), want)
    assert same.all(), f"{name} two={two}: {np.count_nonzero(~same.all(-1))} pixels differ, first (y, x) {np.argwhere(~same.all(-1))[:4].tolist()}"
    assert (got["status"] & INVALID == 0).all() and (got["_pad"] == 0).all()
    if name == "depth 0":
        assert (got["closestRays"] == 0).all() and (got["status"] == 0).all() and np.array_equal(got["seed"], rays["seed"]) and not got["radiance"].any()
    else:
        assert (got["closestRays"] >= 1).all() and 0.1 < (got["status"] == HIT).mean() and ((got["firstT"] > 0) == (got["status"] == HIT)).all()
        assert want.max() > 0
    ps.close()


# ---- anchor 2: chained one-sample calls are the samples of a frame -----------------------------------------------------------------------------
@pytest.mark.parametrize("two", [0, 1], ids=["flat", "two-level"])
@pytest.mark.parametrize("name,samples", [("feature box disney", 3), ("fuzz 2 rtx sun & sky", 2)])
def test_chained_calls_over_the_lens_draws_are_the_samples_of_a_frame(name, samples, two):
    """at aperture 0 every sample of frame 0 shoots the pixel's one ray, after two lens draws: the path loop on seeds rng_tea did not mint"""
    cfg = config(name, max_samples=samples)
    assert cfg.camera.aperture == 0.0
    ps = paths_host.PathScene(cfg)
    st = ps.state()
    calls = chained(ps, two, st, ps.camera_rays(st), samples, skip=2)
    same = same_pixels(mean_of(calls).reshape(cfg.height, cfg.width, 3), oracle_frame0(name, samples)[..., :3])
    assert same.all(), f"{name} two={two}: {np.count_nonzero(~same.all(-1))} pixels differ"
    ps.close()


# ---- composition -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [0, 1], ids=["flat", "two-level"])
@pytest.mark.parametrize("name", ["feature box gltf", "fuzz 2 rtx sun & sky"])
def test_three_samples_in_one_call_are_three_chained_calls(name, two):
    cfg = config(name)
    ps = paths_host.PathScene(cfg)
    st = ps.state(maxSamples=3, fireflyClampThreshold=np.float32(0.5))   # (a threshold that clamps some samples: the clamp is per sample, before the sum)
    rays = ps.camera_rays()
    got = ps.paths(two, st, rays)
    calls = chained(ps, two, st, rays, 3, skip=0)
    assert same_pixels(got["radiance"], mean_of(calls)).all()
    assert np.array_equal(got["seed"], calls[-1]["seed"]) and (calls[0]["seed"] != calls[-1]["seed"]).any()
    assert np.array_equal(got["closestRays"], calls[0]["closestRays"] + calls[1]["closestRays"] + calls[2]["closestRays"])
    assert np.array_equal(bits(got["firstT"]), bits(calls[0]["firstT"])) and np.array_equal(got["status"], calls[0]["status"])
    free = ps.paths(two, ps.state(fireflyClampThreshold=np.float32(np.inf)), rays)
    assert (luma(free["radiance"]) > 0.51).any() and all((luma(c["radiance"]) <= 0.5001).all() for c in calls), "the threshold must clamp some samples"
    ps.close()


# ---- edges -------------------------------------------------------------------------------------------------------------------------------------------
def one_triangle_config(**kw):
    sc, _ = one_triangle_scene()
    return Config(sc, sky(), 8, 8, **kw)


@pytest.mark.parametrize("two", [0, 1], ids=["flat", "two-level"])
def test_depth_extremes_and_a_miss(two):
    ps = paths_host.PathScene(one_triangle_config(hdr_multiplier=3.0))
    rays = make_rays(DEGENERATE_ORG, DEGENERATE_DIR, seeds=[5, 6, 7])   # hit, hit, miss
    # maxDepth 0: nothing is traced
    got = ps.paths(two, ps.state(maxDepth=0, maxSamples=4), rays)
    assert not got["radiance"].any() and np.array_equal(got["seed"], [5, 6, 7]) and (got["closestRays"] == 0).all() and (got["status"] == 0).all() and (got["firstT"] == 0).all()
    # maxDepth 1: one closest-hit ray per sample, whatever it hits
    got = ps.paths(two, ps.state(maxDepth=1, maxSamples=4), rays)
    assert np.array_equal(got["closestRays"], [4, 4, 4]) and np.array_equal(got["status"], [HIT, HIT, 0]) and (got["firstT"][:2] > 0).all() and got["firstT"][2] == 0
    # a miss: the environment along the ray times hdrMultiplier, at any depth; nothing is drawn
    env1 = ps.paths(two, ps.state(maxDepth=5, hdrMultiplier=np.float32(1.0), fireflyClampThreshold=np.float32(np.inf)), rays[2:])
    env3 = ps.paths(two, ps.state(maxDepth=5, hdrMultiplier=np.float32(3.0), fireflyClampThreshold=np.float32(np.inf)), rays[2:])
    assert env1["status"][0] == 0 and env1["seed"][0] == 7 and env1["closestRays"][0] == 1 and (env1["radiance"] > 0).all()
    assert np.array_equal(bits(env3["radiance"]), bits(env1["radiance"] * np.float32(3.0)))
    # closestRays on one triangle: a path that survives leaves the only triangle behind, so every later closest-hit ray is a miss that ends it
    got = ps.paths(two, ps.state(maxDepth=8, maxSamples=16), rays)
    assert (got["closestRays"][:2] >= 16).all() and (got["closestRays"][:2] <= 32).all() and got["closestRays"][2] == 16
    ps.close()


@pytest.mark.parametrize("two", [0, 1], ids=["flat", "two-level"])
def test_firefly_threshold_zero_and_infinite(two):
    cfg = config("feature box disney")
    ps = paths_host.PathScene(cfg)
    rays = ps.camera_rays()
    free = ps.paths(two, ps.state(fireflyClampThreshold=np.float32(np.inf)), rays)
    zero = ps.paths(two, ps.state(fireflyClampThreshold=np.float32(0.0)), rays)
    lum = luma(free["radiance"])
    assert (lum > 0).mean() > 0.5
    # threshold 0: every sample of positive luminance is scaled by 0 / lum; the paths themselves are the same
    assert not zero["radiance"][lum > 0].any() and np.array_equal(zero["seed"], free["seed"]) and np.array_equal(zero["closestRays"], free["closestRays"])
    # +Inf: nothing is clamped -- the default threshold's image with its clamped pixels released
    dflt = ps.paths(two, ps.state(), rays)
    thr = ps.state().fireflyClampThreshold
    keep = ~(lum > np.float32(thr))
    assert np.array_equal(bits(dflt["radiance"][keep]), bits(free["radiance"][keep])) and (luma(dflt["radiance"][~keep]) <= thr * 1.0001).all()
    ps.close()


@pytest.mark.parametrize("two", [0, 1], ids=["flat", "two-level"])
def test_invalid_rays_are_reported_per_ray(two):
    """one ray per rule among valid neighbours; a NaN tmax is no rule here: tmax is ignored"""
    ps = paths_host.PathScene(one_triangle_config())
    st = ps.state(maxDepth=3, maxSamples=2)
    org, dirs, tm, bad = [], [], [], []
    for i, (what, o, d, t, _) in enumerate(invalid_ray_cases()):
        org += [DEGENERATE_ORG[i % 2], o]; dirs += [DEGENERATE_DIR[i % 2], d]; tm += [1e32, t]
        if what != "NaN tmax":
            bad.append(2 * i + 1)
    org.append(DEGENERATE_ORG[1]); dirs.append(DEGENERATE_DIR[1]); tm.append(0.0)   # tmax 0: still unbounded
    rays = make_rays(np.array(org, np.float32), np.array(dirs, np.float32), tmax=np.array(tm, np.float32), seeds=100 + np.arange(len(org)))
    got = ps.paths(two, st, rays)
    bad = np.array(bad); good = np.setdiff1d(np.arange(len(rays)), bad)
    assert len(bad) == 5
    assert (got["status"][bad] == INVALID).all() and np.array_equal(got["seed"][bad], rays["seed"][bad]) and not got["radiance"][bad].any()
    assert (got["firstT"][bad] == 0).all() and (got["closestRays"][bad] == 0).all()
    assert (got["status"][good] == HIT).all() and records_equal(got[good], ps.paths(two, st, rays[good]))   # the neighbours are unaffected
    ps.close()


def test_empty_scenes():
    for sc, _ in empty_scenes():
        ps = paths_host.PathScene(Config(sc, sky(), 8, 8))
        rays = make_rays(DEGENERATE_ORG, DEGENERATE_DIR, seeds=[5, 6, 7])
        for two in (0, 1):
            got = ps.paths(two, ps.state(maxDepth=4, maxSamples=2, fireflyClampThreshold=np.float32(np.inf)), rays)
            assert (got["status"] == 0).all() and np.array_equal(got["closestRays"], [2, 2, 2]) and np.array_equal(got["seed"], [5, 6, 7]) and (got["radiance"] > 0).all()
        ps.close()


def test_segments_are_the_rays_of_the_path():
    """ph_path_segments (what the device tests prove differences with): as many closest-hit rays as the record counts, the first one the caller's ray"""
    cfg = config("feature box disney")
    ps = paths_host.PathScene(cfg)
    st = ps.state(maxSamples=2)
    rays = ps.camera_rays()[::97]
    got = ps.paths(0, st, rays)
    for ray, rec in zip(rays, got):
        seg = ps.segments(0, st, ray)
        closest = seg[seg["seed"] == capi.PT_RAYS_CLOSEST]
        assert len(closest) == rec["closestRays"] and len(seg) - len(closest) <= len(closest)
        assert np.array_equal(bits(closest[0]["origin"]), bits(ray["origin"])) and np.array_equal(bits(closest[0]["direction"]), bits(ray["direction"]))
        assert (seg["tmax"][seg["seed"] == capi.PT_RAYS_OCCLUDED] > 0).all()
    ps.close()


# ---- build -------------------------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_what_its_table_declares():
    if shutil.which("nm") is None:
        pytest.skip("nm is not installed")
    L = paths_host.lib()
    table = [name for name, _, _ in paths_host.SIGNATURES]
    for name in table:
        assert getattr(L, name).argtypes is not None, name
    out = subprocess.run(["nm", "-D", "--defined-only", paths_host.build()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("ph_")}
    assert exported == set(table), (sorted(exported - set(table)), sorted(set(table) - exported))
