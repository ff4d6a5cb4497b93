"""The path loop -- camera_ray, shade_path after the material resolve, finish_bounce_core, accumulate_pixel -- held to the independent float64 model of
tests/golden/gen_path_kat.py, pixel by pixel, through whole frames: 63 images of 46 x 30 pixels of a 32-triangle box.  Each of the five configurations that trace a bounce (disney3, gltf1, rtx3, and
with sun & sky in use sky3 and sky0) has twelve:
the accumulation after 1, 2 and 3 frames and single frames in the last-bounce debug modes eRadiance, eWeight, eRayDir at maxDepth 1, 2, 3.  depth0 (maxDepth 0)
has the three accumulation images only: a debug frame sets maxDepth itself.
sky3 (three lights, hdrMultiplier 0.8, pSelect 0.5) and sky0 (nbLights 0: no pSelect draw, every bounce samples the sun, with two draws where the HDR takes
three) run with SunAndSky::in_use = 1 on the fixture's own SunAndSky words (path_kat_sky.npz holds them and the 24 images): the miss branch
(pathtrace.glsl:219-227), EnvSample's sun branch (env_sampling.glsl:111-125, 133: frame on the RAW sun_direction, one quadrant, pdf 0.5, hdrMultiplier) and the
MIS weight against that constant pdf, all through the sky model of gen_sky_kat.py (tests/test_sky_model.py).  This is what reaches the sun-disk code that
shade_path writes inline.

Legs: the CPU oracle, the compiled reference (pathtrace.comp / pathtrace.rgen), the product's host build flat and two-level.  Each is within 4 x the error the
compiled reference shows against the model (tests/golden/path_kat_tol.json, written by measure_path_kat.py, never taken from the product) on the kept pixels, and
all are bit-identical to each other on every pixel.  tests/test_path_gpu.py holds the device to the same fixture.

PROOF THAT THE CHECK CAN FAIL.  The model was broken one rule at a time (gen_path_kat.BREAK), re-minted in a scratch copy, and the unchanged oracle run against
it; the bound is 4 x the recorded maximum, at most 3.8e-5.  Largest error of the oracle against the broken model, and the image that shows it:
    MIS weight dropped                                             9.99e-01 rtx3_radiance1 (20 of 39 images fail)
    MIS arguments swapped                                          5.74e+00 disney3_radiance3 (20 of 39 images fail)
    pSelect ignored (always 1)                                     7.59e+00 disney3_acc1 (24 of 39 images fail)
    lightPdf 1 for the environment                                 2.15e+00 disney3_radiance1 (20 of 39 images fail)
    NEE not multiplied by throughput                               3.15e+00 disney3_radiance3 (21 of 39 images fail)
    absorption with the wrong sign                                 9.97e-01 gltf1_radiance3 (23 of 39 images fail)
    absorption applied before the emission add                     6.81e-01 disney3_acc1 (21 of 39 images fail)
    roulette without eta * eta                                     8.66e+00 gltf1_radiance3 (27 of 39 images fail)
    roulette constant 0.01 for 0.001                               2.33e+00 disney3_radiance2 (27 of 39 images fail)
    roulette cap 0.9 for 0.95                                      8.61e+00 gltf1_radiance3 (20 of 39 images fail)
    throughput not divided by the continuation probability         8.99e+00 gltf1_radiance3 (27 of 39 images fail)
    no roulette draw when no shadow ray is cast                    9.46e+00 gltf1_acc1 (24 of 39 images fail)
    clamp luminance weights (0.3, 0.6, 0.1)                        3.05e-01 disney3_acc1 (24 of 39 images fail)
    lerp weight 1 / frame                                          5.41e+00 gltf1_acc2 (6 of 39 images fail)
    jitter drawn at frame 0                                        1.10e+01 gltf1_acc1 (36 of 39 images fail)
    tea arguments swapped                                          1.10e+01 gltf1_acc1 (36 of 39 images fail)
    seed not scaled by maxSamples                                  5.48e+00 gltf1_acc2 (2 of 39 images fail)
    offset normal not flipped for transmitted rays                 9.31e+00 gltf1_acc1 (27 of 39 images fail)
and, on the 24 images of sky3 and sky0 (bounds at most 2.2e-4):
    sun pdf 1 for 0.5                                              9.67e-01 sky0_radiance3 (20 of 24 sun & sky images fail)
    sun NEE without hdrMultiplier                                  2.00e-01 sky3_radiance1 (10 of 24 sun & sky images fail: sky0 has hdrMultiplier 1)
    three draws for the sun sample instead of two                  1.50e+02 sky0_acc3 (24 of 24 sun & sky images fail)
    sun_direction normalised before the frame                      1.62e+00 sky0_acc1 (20 of 24 sun & sky images fail)
    sky at a miss without throughput                               2.92e+00 sky3_acc1 (6 of 24 sun & sky images fail: the accumulation images; a debug frame returns no sky)
(The glass slab is emissive so that an emission add occurs while absorption is pending: without that, applying the absorption before the add moves no image.)
The same breaks planted in the product's csrc/pt_shade.h (host build only, scratch copy) against the committed fixture:
    MIS weight dropped                                             4.83e+00 disney3_radiance1 (20 of 39 images fail)
    roulette without eta * eta                                     7.70e+00 gltf1_acc1 (27 of 39 images fail)
    offset normal not flipped for transmitted rays                 1.26e+01 gltf1_acc1 (27 of 39 images fail)
    RNG state not written back at the last-bounce debug exit       6.77e+00 gltf1_weight2 (18 of 39 images fail)
    sun pdf 1 for 0.5                                              4.94e-01 sky0_radiance3 (20 of 24 sun & sky images fail)
    sun NEE without hdrMultiplier                                  2.50e-01 sky3_radiance1 (10 of 24 sun & sky images fail)
    sun_direction normalised before the frame                      1.00e+00 sky0_acc1 (20 of 24 sun & sky images fail)
    sky at a miss without throughput                               1.22e+00 sky3_acc1 (6 of 24 sun & sky images fail)
The sun & sky images found nothing in the product: every leg is within its bound on them and all are bit-identical.
"RNG state not written back" is the bug these tests found in shade_path: the exit returned without storing the seed, so the second sample of a frame continued from the seed
the bounce began with (host build and device alike; oracle and reference were right).  All eighteen debug images of the two maxSamples = 2 configurations,
ray query and RTX, fail on it, and the host build differs from the oracle on 774 of 1380 pixels of rtx3_radiance1.  pt_shade.h now stores the seed there.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import orc, path_kat_io as io, ref
from vk_raytrace_amd import capi, host_device as hd


@pytest.fixture(scope="module")
def kat():
    return io.load()


@pytest.fixture(scope="module")
def gen():
    return io.generator()


@pytest.fixture(scope="module")
def tol():
    return io.tolerances()


def rendered(kat, leg):
    out = dict(io.render_all(kat, leg))
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def oracle_out(kat):
    return rendered(kat, io.oracle)


@pytest.fixture(scope="module")
def host_out(kat):
    return rendered(kat, io.host(0)), rendered(kat, io.host(1))


def test_generator_is_independent_and_deterministic(tmp_path, gen):
    src = open(os.path.join(io.GOLDEN, "gen_path_kat.py")).read()
    imports = re.findall(r"^\s*(?:from|import)\s+([\w.]+)", src, re.M)
    assert set(imports) <= {"os", "sys", "numpy", "gen_kat", "gen_float_kat", "gen_sky_kat", "gen_surface_kat", "gen_tex_kat"}, imports   # nothing of oracle/, tests/, vk_raytrace_amd/
    assert len(re.findall(r"#.*?:\d+(-\d+)?", src)) >= 30   # shader lines cited per rule
    out = str(tmp_path / "again.npz")
    gen.main(out)
    # both files: the 39 images without sun & sky (expectations and kept masks as they were before sky3 and sky0 joined) and the 24 with it
    # (When sky3 and sky0 were added, the arrays of the re-minted path_kat.npz were compared once with those of the file committed before: all 142 are equal byte
    # for byte except tag_names, which grew from 38 to 48 entries; the 39 entries of path_kat_tol.json did not change either.)
    mine = ("path_kat.npz", "path_kat_sky.npz")
    largest = 974864   # bytes of display_kat.npz, the largest file of tests/golden/ before the sun & sky fixtures were added
    for again, committed in zip((out, out[:-4] + "_sky.npz"), mine):
        assert open(again, "rb").read() == open(os.path.join(io.GOLDEN, committed), "rb").read(), committed
        assert os.path.getsize(again) <= largest


def test_fixture_meets_the_caps(kat, gen, tol):
    """at most 10 % of an image dropped, at least 50 kept pixels per branch class (the generator's tags), every expectation finite where kept; the scene is as
    small as the issue asks and draws nothing in traversal"""
    worst, counts = gen.check_caps(kat)
    assert worst <= 0.10 and (counts >= 50).all()
    assert list(kat["tag_names"]) == list(gen.TAGS)
    assert np.array_equal(kat["env"], gen.environment()) and kat["env_table"].shape == (kat["env"].shape[0] * kat["env"].shape[1], 4)
    assert np.array_equal(kat["sunsky"], gen.sunsky()) and kat["sunsky"].view(np.int32)[23] == 1 and list(kat["sky_config_names"]) == list(gen.SKY_CONFIGS)
    assert kat["cfg_sky0"][0] == 0 and kat["cfg_sky3"][0] == 3 and kat["cfg_sky3"][1] > 0 and len(kat["image_names"]) == 63
    for cn in ("disney3", "gltf1", "rtx3", "sky3", "sky0"):   # every configuration that traces a bounce has all twelve observables
        assert {f"{cn}_acc{k}" for k in (1, 2, 3)} | {f"{cn}_{m}{k}" for m in ("radiance", "weight", "raydir") for k in (1, 2, 3)} <= set(kat["image_names"])
    for name in kat["image_names"]:
        assert np.isfinite(kat["img_" + name][kat["kept_" + name]]).all()
        assert tol[str(name)]["kept"] == int(kat["kept_" + name].sum()), "path_kat_tol.json was measured on another fixture"
        assert tol[str(name)]["max"] <= 1e-3
    assert len(kat["indices"]) // 3 <= 32
    m = kat["materials"]
    assert (m["alphaMode"] == hd.ALPHA_OPAQUE).all() and (m["pbrBaseColorTexture"] == -1).all() and (m["normalTexture"] == -1).all()
    w, h = kat["size"]
    assert w % 8 and h % 8 and w % hd.TILE and h % hd.TILE


def test_every_legs_alias_table_is_the_fixtures(kat):
    env = np.ascontiguousarray(kat["env"], np.float32)
    h, w = env.shape[:2]
    want = kat["env_table"].tobytes()
    acc = np.zeros(w * h, hd.envaccel_dtype)
    i, a = C.c_float(), C.c_float()
    orc.lib().orc_build_env_accel(env.ctypes.data, w, h, acc.ctypes.data, C.byref(i), C.byref(a))
    assert acc.tobytes() == want and np.float32(i.value) == kat["env_integral"] and np.float32(a.value) == kat["env_average"]
    acc, i, a = capi.build_env_accel(env)
    assert acc.tobytes() == want and np.float32(i) == kat["env_integral"] and np.float32(a) == kat["env_average"]
    if ref.available():
        acc = np.zeros(w * h, hd.envaccel_dtype)
        i, a = C.c_float(), C.c_float()
        assert ref.lib().ref_env_accel(env.ctypes.data, w, h, acc.ctypes.data, C.byref(i), C.byref(a)) == w * h
        assert acc.tobytes() == want and np.float32(i.value) == kat["env_integral"]


def test_oracle_within_the_bound(kat, tol, oracle_out):
    for name, img in oracle_out.items():
        io.check(kat, tol, name, img)


@pytest.mark.skipif(not ref.available(), reason="needs the reference tree (or a prebuilt oracle/_ref/libref.so)")
def test_reference_within_the_bound_and_equal_to_the_oracle(kat, tol, oracle_out):
    for name, img in io.render_all(kat, io.reference):
        io.check(kat, tol, name, img)
        assert io.same_bits(img, oracle_out[name]), name


def test_host_build_within_the_bound(kat, tol, host_out):
    for out in host_out:
        for name, img in out.items():
            io.check(kat, tol, name, img)


def test_legs_are_bit_identical(kat, oracle_out, host_out):
    """every pixel, kept or not"""
    for name, img in oracle_out.items():
        assert io.same_bits(host_out[0][name], img), f"{name}: host build (flat) differs from the oracle"
        assert io.same_bits(host_out[1][name], img), f"{name}: host build (two-level) differs from the oracle"
