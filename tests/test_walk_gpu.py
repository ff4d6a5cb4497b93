"""The device legs of tests/test_walk_model.py: the fixture of tests/golden/gen_walk_kat.py through pt_trace_rays on the device, every record held to the model by
the rules of tests/walk_kat_io.py AND to the query host build bit for bit -- CLOSEST, OCCLUDED in both variants, CANDIDATES with 16 results, the flat and the
two-level structure, pt_use_any_hit(0), for the first 4 097 rays and for the whole set.  The zero-draw rays (a draw of exactly 0.0) lie inside the first 4 097:
rays 128 .. 191 are one wavefront of nothing else, the others share their wavefronts with ordinary rays (test_zero_draw_rays_sit_where_the_device_test_needs_them).

One frames case reaches the kernels the C ABI cannot seed (the trace machine's lane_settle, k_closest_k, k_tail's bodies, the queueX route into the exact
kernels): the fixture scene behind one screen-filling BLEND card of factor 0, 64 x 64, maxDepth 2, maxSamples 1, at the first frame index whose seeds give some
pixel a first traversal draw of exactly 0.0.  That is frame 712, pixel 1230 (x 14, y 19) -- walk_kat_io.first_zero_frame computes it from tea and samplePixel's
draw order, and the test asserts it.  There the card commits; everywhere else it is rejected."""
import os

import numpy as np
import pytest

from tests import walk_kat_io as io
from tests.host_harness import TracedScene
from tests.test_query_host import CANDIDATES, CLOSEST, OCCLUDED, host_query, records_equal
from vk_raytrace_amd import capi, host_device as hd
from vk_raytrace_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu
ACCELS = [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL]
ACCEL_IDS = ["flat", "two-level"]
VARIANTS = (capi.PT_VARIANT_RAYQUERY, capi.PT_VARIANT_RTX)
FRAME, PIXEL = 712, 1230


@pytest.fixture(scope="module")
def kat():
    return io.load()


def renderer(scene, accel):
    r = HipRenderer()
    r.setup(0)
    r.set_accel_mode(accel)
    r.set_scene(scene)
    return r


@pytest.mark.parametrize("n", [4097, None], ids=["4097 rays", "all rays"])
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_trace_rays_against_the_model_and_the_host_build(kat, accel, n):
    two = 1 if accel == capi.PT_ACCEL_TWO_LEVEL else 0
    sc = io.fixture_scene(kat)
    tr, r = TracedScene(sc), renderer(sc, accel)
    rays = io.rays(kat, n)
    what = f"device {ACCEL_IDS[two]} n={len(rays)}"
    try:
        dev = r.trace_ray_records(CLOSEST, rays)
        answered = io.records_closest(kat, what + " CLOSEST", dev)
        assert records_equal(dev, host_query(tr, two, CLOSEST, rays)), what + " CLOSEST: records off the host build"
        for variant in VARIANTS:
            r.set_variant(variant)
            dev = r.trace_ray_records(OCCLUDED, rays)
            answered &= io.records_shadow(kat, what + f" OCCLUDED variant {variant}", dev, variant)
            assert records_equal(dev, host_query(tr, two, OCCLUDED, rays, variant=variant)), what + f" OCCLUDED variant {variant}: records off the host build"
        r.set_variant(capi.PT_VARIANT_RAYQUERY)
        dev = r.trace_ray_records(CANDIDATES, rays, io.KEYS)
        answered &= io.records_candidates(kat, what + " CANDIDATES", dev)
        assert records_equal(dev, host_query(tr, two, CANDIDATES, rays, hits_per_ray=io.KEYS)), what + " CANDIDATES: records off the host build"
        if n is None:
            io.census(kat, answered)
        else:   # the first 4 097 rays hold every zero-draw ray and every exact row
            zero = (kat["ray_family"][:n] == io.F_ZERO) & answered
            assert zero.sum() == (kat["ray_family"] == io.F_ZERO).sum() and zero[128:192].all()
        # pt_use_any_hit(0): every triangle opaque, nothing draws
        r.useAnyHit(False)
        io.records_closest(kat, what + " any-hit off CLOSEST", r.trace_ray_records(CLOSEST, rays), opaque=True)
        for variant in VARIANTS:
            r.set_variant(variant)
            io.records_shadow(kat, what + " any-hit off OCCLUDED", r.trace_ray_records(OCCLUDED, rays), variant, opaque=True)
        io.records_candidates(kat, what + " any-hit off CANDIDATES", r.trace_ray_records(CANDIDATES, rays, io.KEYS))
    finally:
        r.destroy(); tr.close()


def oracle_frame(cfg, frame):
    from tests import orc
    o = orc.Oracle()
    o.set_scene(cfg.scene)
    integral, _ = o.set_env(cfg.env)
    o.set_camera(cfg.camera)
    o.set_sunsky(cfg.sunsky)
    img = o.render(cfg.state(integral), 1, first_frame=frame)
    stats = o.stats()
    o.close()
    return img, stats


def device_frame(cfg, frame, accel, tune):
    keep = os.environ.get("PT_TUNE")
    os.environ["PT_TUNE"] = tune          # (pt_create reads the launch policy)
    try:
        r = HipRenderer()
        r.setup(0)
    finally:
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
        st = cfg.state(integral)
        st.frame = frame
        r.setPushContants(st)
        r.run(None, (cfg.width, cfg.height), None, None)
        return r.read_accum(), r.stats()
    finally:
        r.destroy()


@pytest.fixture(scope="module")
def frame_reference(kat):
    frame, pixels = io.first_zero_frame()
    assert (frame, list(pixels)) == (FRAME, [PIXEL]), "the frame index the docstring names"
    return {debug: oracle_frame(io.frames_config(kat, debug), frame) for debug in (0, hd.eBaseColor, hd.eAlpha)}


@pytest.mark.parametrize("tune", ["tail=0", "tail=0,fuse=0", "tail=1000000000", "tail=0,packetClosest=0"])
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
def test_the_zero_draw_in_a_frame(kat, frame_reference, accel, tune):
    """frame 712 alone, under four launch policies: the accumulation image equals the oracle's bit for bit, alphaTests and closestRays equal the oracle's, and the
    model's first-hit verdict for pixel 1230 -- the card commits, nowhere else -- is what the eBaseColor / eAlpha images of the same frame show"""
    want, want_stats = frame_reference[0]
    assert want_stats["alphaTests"] >= io.FRAME_SIZE ** 2 and np.isfinite(want).all() and want[..., :3].max() > 0
    got, stats = device_frame(io.frames_config(kat), FRAME, accel, tune)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{tune}: {np.count_nonzero((got.view(np.uint32) != want.view(np.uint32)).any(-1))} pixels differ from the oracle"
    for k in ("alphaTests", "closestRays"):
        assert stats[k] == want_stats[k], (k, stats[k], want_stats[k])
    base, _ = device_frame(io.frames_config(kat, hd.eBaseColor), FRAME, accel, tune)
    assert list(io.card_pixels(base, FRAME)) == [PIXEL] and np.array_equal(base.view(np.uint32), frame_reference[hd.eBaseColor][0].view(np.uint32))
    alpha, _ = device_frame(io.frames_config(kat, hd.eAlpha), FRAME, accel, tune)
    assert np.array_equal(alpha.view(np.uint32), frame_reference[hd.eAlpha][0].view(np.uint32))
    assert alpha[..., 0].reshape(-1)[PIXEL] == 0.0, "the card's alpha is 0"   # (a miss shows 0 too: the base-colour image is what singles the card out)
