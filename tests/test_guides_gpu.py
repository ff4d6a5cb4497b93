"""The guide pass on the device (pt_render_guides / pt_read_denoise_guides through the C ABI) against the host build of the same header
(tests/guides_host.py), which tests/test_guides_host.py holds to the oracle: device == host bit for bit on every pixel of every plane, on the flat
structure with and without the per-slot shading lines and on the two-level one; against the composed route (render_guides: debug frames +
pt_trace_rays) it replaces; as the denoiser's input; without side effects on a frame sequence; plane masks, a sharded context, errors."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from tests import denoise_host as dh, guides_host
from tests import test_guides_host as host
from tests.common import Config, render_hip
from tests.host_harness import TracedScene
from vk_raytrace_amd import capi, host_device as hd, synth
from vk_raytrace_amd.renderer import HipRenderer
from vk_raytrace_amd.scene import Camera, Scene, rotate_y, translate

pytestmark = pytest.mark.gpu
SIZES, APERTURES, MISS_DEPTH, bits = host.SIZES, host.APERTURES, host.MISS_DEPTH, host.bits
ENV = synth.procedural_sky(64, 32)


@contextlib.contextmanager
def tuning(value):
    """PT_TUNE for the contexts created inside (the knobs are read at pt_create)"""
    old = os.environ.get("PT_TUNE")
    if value is not None:
        os.environ["PT_TUNE"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("PT_TUNE", None)
        else:
            os.environ["PT_TUNE"] = old


def open_renderer(scene, size=None, accel=None, tune=None, shard=None):
    with tuning(tune):
        r = HipRenderer()
        r.setup(0)
    if accel is not None:
        r.set_accel_mode(accel)
    if shard is not None:
        r.set_shard(*shard)
    if scene is not None:
        r.set_scene(scene)
    r.set_env(ENV)
    r.set_sunsky(hd.default_sun_and_sky())
    if size is not None:
        r.create(size)
        if scene is not None:
            r.set_camera(host.camera_for(scene, size[0], size[1], 0.0))
    return r


def opaque_scene():
    """a diffuse floor, a back wall and two boxes: nothing with alpha, sky above the wall"""
    sc = Scene("guides_opaque")
    mats = [sc.add_material(pbrBaseColorFactor=c + (1,), pbrMetallicFactor=0.0, pbrRoughnessFactor=1.0) for c in ((0.7, 0.7, 0.7), (0.8, 0.25, 0.2), (0.2, 0.6, 0.3))]
    synth._add(sc, synth.grid(4, 4, (-3, 0, 3), (6, 0, 0), (0, 0, -6)), mats[0])
    synth._add(sc, synth.grid(4, 3, (-3, 0, -2), (6, 0, 0), (0, 1.5, 0)), mats[0])
    synth._add(sc, synth.box((0.8, 1.2, 0.8)), mats[1], translate(-1.0, 0.6, -0.6) @ rotate_y(0.5))
    synth._add(sc, synth.box((0.9, 0.7, 0.9)), mats[2], translate(0.4, 0.35, 0.2) @ rotate_y(-0.3))
    sc.camera = Camera(eye=(0.0, 1.6, 3.4), center=(0.0, 0.9, -0.5), up=(0, 1, 0), fov=50.0)
    sc.finalize(capi.pack_vertices)
    return sc


def assert_planes_equal(got, want, what):
    for j in range(3):
        same = (bits(got[j]) == bits(want[j])).all(-1)
        assert same.all(), f"{what}: plane {j} differs at {np.count_nonzero(~same)} pixels, first (y, x) {np.argwhere(~same)[:4].tolist()}"


# ---- 1. device against the host build -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", host.ALPHA_SCENES)
def test_device_equals_the_host_build_bit_for_bit(name):
    """flat with the per-slot shading lines (the default), flat without them (PT_TUNE shadeTris=0), two-level; both sizes, pinhole and aperture"""
    c = host.case(name)
    want = {}
    for (w, h) in SIZES:
        for ap in APERTURES:
            c.set_camera(w, h, ap)
            for two in (0, 1):
                want[w, h, ap, two] = guides_host.guides(c.traced, two, w, h, 7, MISS_DEPTH)
    for what, accel, tune in (("flat", capi.PT_ACCEL_FLAT, None), ("flat, shadeTris=0", capi.PT_ACCEL_FLAT, "shadeTris=0"), ("two-level", capi.PT_ACCEL_TWO_LEVEL, None)):
        r = open_renderer(c.scene, accel=accel, tune=tune)
        try:
            for (w, h) in SIZES:
                r.create((w, h))
                for ap in APERTURES:
                    r.set_camera(host.camera_for(c.scene, w, h, ap))
                    r.capture_guides(7, MISS_DEPTH)
                    assert_planes_equal(r.read_guides(), want[w, h, ap, int(accel == capi.PT_ACCEL_TWO_LEVEL)], f"{name} {what} {w}x{h} aperture {ap}")
        finally:
            r.destroy()


# ---- 2. device against the composed route ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aperture", APERTURES)
def test_colour_and_normal_are_the_planes_of_the_composed_route(aperture):
    """render_guides -- two frame-0 debug frames through the whole launch sequence -- returns the planes the pass writes (its depth plane is the
    pinhole ray's with seed 0: not compared)"""
    sc = host.case("fuzz1").scene
    w, h = SIZES[1]
    r = open_renderer(sc, (w, h))
    try:
        r.set_camera(host.camera_for(sc, w, h, aperture))
        composed = r.render_guides(host.guide_state(w, h, 0))
        r.capture_guides(7, 1e30)
        got = r.read_guides()
        for j in (0, 1):
            assert np.array_equal(bits(got[j]), bits(composed[j])), j
        assert (got[2][..., 0] < 1e30).mean() > 0.1
    finally:
        r.destroy()


def test_depth_is_pt_trace_rays_on_the_same_rays():
    """opaque scene, pinhole: plane 2 is the closest-hit distance pt_trace_rays reports for the host build's camera rays"""
    sc = opaque_scene()
    w, h = SIZES[1]
    tr = TracedScene(sc)
    guides_host.set_camera(tr, host.camera_for(sc, w, h, 0.0))
    org, dirs, s_cam, s_walk = guides_host.rays(tr, w, h)
    tr.close()
    assert np.array_equal(s_cam, s_walk)
    r = open_renderer(sc, (w, h))
    try:
        hits = r.trace_rays(capi.PT_RAYS_CLOSEST, org, dirs, seeds=s_cam)
        hit = (hits["status"] & capi.PT_RAY_HIT) != 0
        assert 0.1 < hit.mean() < 0.9
        r.capture_guides(capi.PT_GUIDES_DEPTH, MISS_DEPTH)
        depth = r.read_guides(capi.PT_GUIDES_DEPTH)[2]
        assert np.array_equal(bits(depth[..., 0].reshape(-1)), bits(np.where(hit, hits["t"], np.float32(MISS_DEPTH)).astype(np.float32)))
        assert not bits(depth[..., 1:]).any()
    finally:
        r.destroy()


# ---- 3. denoiser input ----------------------------------------------------------------------------------------------------------------------------------
def test_the_denoiser_reads_the_planes_in_place_as_it_reads_uploaded_ones():
    sc = host.case("fuzz5").scene
    w, h = SIZES[1]
    r = open_renderer(sc, (w, h))
    try:
        rng = np.random.default_rng(3)
        colour = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), (h, w, 4))).astype(np.float32)
        r.write_accum(colour)
        p = dh.params(3, 1.5, (0.1, 0.3, 0.5), capi.PT_DENOISE_DEMODULATE)
        tm = hd.default_tonemapper()
        r.capture_guides(7, 100.0)
        den, shown = r.denoise(p), r.tonemap_denoised(p, tm)
        planes = r.read_guides()
        r.set_denoise_guides(None, None, None)
        r.set_denoise_guides(*planes)
        assert np.array_equal(bits(r.denoise(p)), bits(den)) and np.array_equal(r.tonemap_denoised(p, tm), shown)
        rc, want = dh.denoise(colour, planes, p)
        assert rc == 0 and np.array_equal(bits(den), bits(want))
        assert not np.array_equal(bits(den), bits(colour))
    finally:
        r.destroy()


# ---- 4. no side effects ---------------------------------------------------------------------------------------------------------------------------------
def test_a_frame_sequence_with_guide_passes_in_between_continues_bit_for_bit():
    """six frames with pt_render_guides after frames 0, 2 and 3 and no synchronisation in between: accumulation image and counters of the uninterrupted
    run; a frame after pt_read_denoise_guides continues the running mean"""
    cfg = Config(synth.feature_box(tex_size=32), ENV, 64, 48)
    results = []
    for interrupt in (False, True):
        r = open_renderer(cfg.scene, (64, 48))
        r.set_camera(cfg.camera)
        st = cfg.state(r.env_integral)
        r.reset_stats()
        for f in range(6):
            st.frame = f
            r.setPushContants(st)
            r.run()
            if interrupt and f in (0, 2, 3):
                r.capture_guides()
        img = r.read_accum()
        stats = {k: v for k, v in r.stats().items() if not k.startswith("ms")}
        if interrupt:
            planes = r.read_guides()
            assert (planes[2][..., 0] < 1e30).any() and planes[0][..., :3].max() > 0
        st.frame = 6
        r.setPushContants(st)
        r.run()
        results.append((img, stats, r.read_accum()))
        r.destroy()
    (img_a, stats_a, next_a), (img_b, stats_b, next_b) = results
    assert np.array_equal(bits(img_a), bits(img_b)) and stats_a == stats_b and stats_a["samples"] == 6 * 64 * 48
    assert np.array_equal(bits(next_a), bits(next_b)) and np.array_equal(bits(next_b), bits(render_hip(cfg, 7)))


# ---- 5. plane masks -------------------------------------------------------------------------------------------------------------------------------------
def test_plane_masks_and_resize():
    sc = opaque_scene()
    w, h = SIZES[1]
    r = open_renderer(sc, (w, h))
    try:
        r.capture_guides(7, MISS_DEPTH)
        full = r.read_guides()
        mine = np.full((h, w, 4), 0.375, np.float32)
        # an installed plane outside the mask survives, one inside it is replaced, an unset one outside it stays unset
        r.set_denoise_guides(mine, mine, None)
        r.capture_guides(capi.PT_GUIDES_NORMAL, MISS_DEPTH)
        got = r.read_guides(capi.PT_GUIDES_BASECOLOR | capi.PT_GUIDES_NORMAL)
        assert np.array_equal(got[0], mine) and np.array_equal(bits(got[1]), bits(full[1])) and got[2] is None
        with pytest.raises(capi.PtError) as e:
            r.read_guides(capi.PT_GUIDES_DEPTH)
        assert e.value.code == capi.PT_ERR_STATE
        with pytest.raises(capi.PtError) as e:
            r.read_guides()
        assert e.value.code == capi.PT_ERR_STATE
        r.capture_guides(capi.PT_GUIDES_DEPTH, MISS_DEPTH)
        got = r.read_guides()
        assert np.array_equal(got[0], mine) and np.array_equal(bits(got[1]), bits(full[1])) and np.array_equal(bits(got[2]), bits(full[2]))
        # a resize to the same size keeps them (as it keeps installed planes), one to another size drops all of them
        r.create((w, h))
        assert np.array_equal(bits(r.read_guides()[2]), bits(full[2]))
        r.set_denoise_guides(mine, None, None)
        r.create((w, h))
        assert np.array_equal(r.read_guides(capi.PT_GUIDES_BASECOLOR)[0], mine)
        r.capture_guides(7, MISS_DEPTH)
        r.create((w + 3, h))
        for j in range(3):
            with pytest.raises(capi.PtError) as e:
                r.read_guides(1 << j)
            assert e.value.code == capi.PT_ERR_STATE
        r.set_camera(host.camera_for(sc, w + 3, h, 0.0))
        r.capture_guides(capi.PT_GUIDES_BASECOLOR)
        assert r.read_guides(capi.PT_GUIDES_BASECOLOR)[0].shape == (h, w + 3, 4)
    finally:
        r.destroy()


# ---- 6. sharded context ---------------------------------------------------------------------------------------------------------------------------------
def test_a_sharded_context_renders_the_whole_image():
    sc = host.case("fuzz0").scene
    w, h = SIZES[0]     # 3 x 2 tiles of 32 x 32: rank 1 of 2 owns three of them
    planes = []
    for shard in (None, (1, 2)):
        r = open_renderer(sc, (w, h), shard=shard)
        try:
            r.capture_guides(7, MISS_DEPTH)
            planes.append(r.read_guides())
        finally:
            r.destroy()
    assert_planes_equal(planes[1], planes[0], "rank 1 of 2")
    assert (planes[0][2][..., 0] != np.float32(MISS_DEPTH)).any()


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    L = capi.lib()
    sc = opaque_scene()
    w, h = SIZES[1]
    out = [np.zeros((h, w, 4), np.float32) for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
    # before a scene / an acceleration structure, before a camera, before a size
    r = open_renderer(None, (w, h))
    try:
        assert L.pt_render_guides(r._ctx, 7, 1.0) == capi.PT_ERR_STATE and b"pt_build_accel" in L.pt_last_error(r._ctx)
        r.set_scene(sc)
        assert L.pt_render_guides(r._ctx, 7, 1.0) == capi.PT_ERR_STATE and b"pt_set_camera" in L.pt_last_error(r._ctx)
    finally:
        r.destroy()
    r = open_renderer(sc)
    try:
        r.set_camera(host.camera_for(sc, w, h, 0.0))
        assert L.pt_render_guides(r._ctx, 7, 1.0) == capi.PT_ERR_STATE and b"pt_resize" in L.pt_last_error(r._ctx)
        assert L.pt_read_denoise_guides(r._ctx, ptrs) == capi.PT_ERR_STATE and b"pt_resize" in L.pt_last_error(r._ctx)
        r.create((w, h))
        assert L.pt_read_denoise_guides(r._ctx, ptrs) == capi.PT_ERR_STATE   # nothing installed
        assert L.pt_read_denoise_guides(r._ctx, None) == capi.PT_ERR_INVALID
        assert L.pt_render_guides(None, 7, 1.0) == capi.PT_ERR_INVALID and L.pt_read_denoise_guides(None, ptrs) == capi.PT_ERR_INVALID
        r.capture_guides(7, MISS_DEPTH)
        before = r.read_guides()
        # arguments: nothing is launched, the planes stay what they were
        for planes, miss in ((0, 1.0), (8, 1.0), (15, 1.0), (7, float("nan")), (7, float("inf")), (7, float("-inf"))):
            assert L.pt_render_guides(r._ctx, planes, miss) == capi.PT_ERR_INVALID, (planes, miss)
        assert_planes_equal(r.read_guides(), before, "after refused calls")
        none = (C.c_void_p * 3)(None, None, None)
        assert L.pt_read_denoise_guides(r._ctx, none) == capi.PT_OK   # nothing asked for
    finally:
        r.destroy()


def test_an_overflow_of_its_walks_is_reported_by_the_next_synchronising_call():
    """the overflow scene and camera of tests/test_gpu_edges.py: the camera walks need more than 64 stack entries; the pass itself returns PT_OK
    (asynchronous), pt_read_denoise_guides and pt_synchronize report it, pt_reset_stats clears it"""
    deep = Config(synth.deep_chain(synth.DEEP_OVERFLOW_LEVELS), ENV, 32, 24, depth=2)
    r = open_renderer(deep.scene, (32, 24))
    try:
        r.set_camera(deep.camera)
        r.capture_guides()
        for fn in (r.read_guides, r.synchronize):
            with pytest.raises(capi.PtError) as e:
                fn()
            assert e.value.code == capi.PT_ERR_STATE and "overflowed" in str(e.value)
        r.reset_stats()
        r.synchronize()
    finally:
        r.destroy()
