"""The instance pass on the device (pt_render_instance_plane / pt_read_instance_plane / pt_set_instance_plane through the C ABI)
against the host build of the same functions (tests/motion_host.py), which tests/test_instances_host.py holds to the oracle: the instance plane and the
guide planes written alongside equal the host's bit for bit -- and the guide planes are pt_render_guides' -- on the flat structure with and without the
per-slot shading lines and on the two-level one; the plane against pt_trace_rays; no side effects on a frame sequence; the setter and the read-back;
errors, and a mask of 0."""
import numpy as np
import pytest

from tests import guides_host, motion_host as mh
from tests import test_guides_gpu as gg
from tests import test_guides_host as host
from tests.common import Config, render_hip
from tests.host_harness import TracedScene
from vk_raytrace_amd import capi, synth

pytestmark = pytest.mark.gpu
SIZES, APERTURES, MISS_DEPTH, bits = host.SIZES, host.APERTURES, host.MISS_DEPTH, host.bits
MODES = (("flat", capi.PT_ACCEL_FLAT, None), ("flat, shadeTris=0", capi.PT_ACCEL_FLAT, "shadeTris=0"), ("two-level", capi.PT_ACCEL_TWO_LEVEL, None))


def assert_ids_equal(got, want, what):
    same = got == want
    assert same.all(), f"{what}: the instance plane differs at {np.count_nonzero(~same)} pixels, first (y, x) {np.argwhere(~same)[:4].tolist()}"


@pytest.mark.parametrize("name", host.ALPHA_SCENES)
def test_device_equals_the_host_build_bit_for_bit(name):
    """flat with the per-slot shading lines (the default), flat without them (PT_TUNE shadeTris=0), two-level; both sizes, pinhole and aperture: the
    instance plane and all three guide planes; the guide planes are also what pt_render_guides leaves"""
    c = host.case(name)
    want = {}
    for (w, h) in SIZES:
        for ap in APERTURES:
            c.set_camera(w, h, ap)
            for two in (0, 1):
                want[w, h, ap, two] = mh.instances(c.traced, two, w, h, 7, MISS_DEPTH)
    for what, accel, tune in MODES:
        r = gg.open_renderer(c.scene, accel=accel, tune=tune)
        try:
            for (w, h) in SIZES:
                r.create((w, h))
                for ap in APERTURES:
                    r.set_camera(host.camera_for(c.scene, w, h, ap))
                    r.render_instance_plane(7, MISS_DEPTH)
                    ids, planes = want[w, h, ap, int(accel == capi.PT_ACCEL_TWO_LEVEL)]
                    label = f"{name} {what} {w}x{h} aperture {ap}"
                    assert_ids_equal(r.read_instance_plane(), ids, label)
                    got = r.read_guides()
                    gg.assert_planes_equal(got, planes, label)
                    r.capture_guides(7, MISS_DEPTH)
                    gg.assert_planes_equal(r.read_guides(), got, label + " (pt_render_guides)")
                    hit = ids != capi.PT_INSTANCE_NONE
                    assert (ids[hit] < len(c.scene.nodes)).all() and np.array_equal(hit, got[2][..., 0] != np.float32(MISS_DEPTH))
        finally:
            r.destroy()


@pytest.mark.parametrize("what,accel,tune", MODES, ids=[m[0] for m in MODES])
def test_the_plane_is_pt_trace_rays_instance_of_the_same_rays(what, accel, tune):
    """opaque scene, pinhole: the plane holds the instanceID pt_trace_rays(CLOSEST) reports for the host build's camera rays, 0xffffffff for a miss"""
    sc = gg.opaque_scene()
    w, h = SIZES[1]
    tr = TracedScene(sc)
    guides_host.set_camera(tr, host.camera_for(sc, w, h, 0.0))
    org, dirs, s_cam, _ = guides_host.rays(tr, w, h)
    tr.close()
    r = gg.open_renderer(sc, (w, h), accel=accel, tune=tune)
    try:
        hits = r.trace_rays(capi.PT_RAYS_CLOSEST, org, dirs, seeds=s_cam)
        r.render_instance_plane(0)
        ids = r.read_instance_plane()
        assert_ids_equal(ids.reshape(-1), hits["instanceID"], what)
        assert set(np.unique(ids).tolist()) == {0, 1, 2, 3, capi.PT_INSTANCE_NONE}      # floor, wall, both boxes and the sky
    finally:
        r.destroy()


def test_a_frame_sequence_with_instance_passes_in_between_continues_bit_for_bit():
    """six frames with pt_render_instance_plane after frames 0, 2 and 3 and no synchronisation in between: accumulation image and counters of the
    uninterrupted run; a frame after pt_read_instance_plane continues the running mean"""
    cfg = Config(synth.feature_box(tex_size=32), gg.ENV, 64, 48)
    results = []
    for interrupt in (False, True):
        r = gg.open_renderer(cfg.scene, (64, 48))
        r.set_camera(cfg.camera)
        st = cfg.state(r.env_integral)
        r.reset_stats()
        for f in range(6):
            st.frame = f
            r.setPushContants(st)
            r.run()
            if interrupt and f in (0, 2, 3):
                r.render_instance_plane(7 if f else 0)
        img = r.read_accum()
        stats = {k: v for k, v in r.stats().items() if not k.startswith("ms")}
        if interrupt:
            ids = r.read_instance_plane()
            assert (ids != capi.PT_INSTANCE_NONE).any() and (r.read_guides()[2][..., 0] < 1e30).any()
        st.frame = 6
        r.setPushContants(st)
        r.run()
        results.append((img, stats, r.read_accum()))
        r.destroy()
    (img_a, stats_a, next_a), (img_b, stats_b, next_b) = results
    assert np.array_equal(bits(img_a), bits(img_b)) and stats_a == stats_b and stats_a["samples"] == 6 * 64 * 48
    assert np.array_equal(bits(next_a), bits(next_b)) and np.array_equal(bits(next_b), bits(render_hip(cfg, 7)))


def test_a_mask_of_zero_the_setter_and_resize():
    sc = gg.opaque_scene()
    w, h = SIZES[1]
    r = gg.open_renderer(sc, (w, h))
    try:
        # mask 0: the plane alone; installed guide planes stay as they are, unset ones stay unset
        mine = np.full((h, w, 4), 0.375, np.float32)
        r.set_denoise_guides(mine, None, None)
        r.render_instance_plane(0, MISS_DEPTH)
        ids = r.read_instance_plane()
        assert np.array_equal(r.read_guides(capi.PT_GUIDES_BASECOLOR)[0], mine)
        with pytest.raises(capi.PtError) as e:
            r.read_guides(capi.PT_GUIDES_DEPTH)
        assert e.value.code == capi.PT_ERR_STATE
        # a mask of one plane writes that plane, and the same instance plane
        r.render_instance_plane(capi.PT_GUIDES_DEPTH, MISS_DEPTH)
        assert_ids_equal(r.read_instance_plane(), ids, "mask 4")
        got = r.read_guides(capi.PT_GUIDES_BASECOLOR | capi.PT_GUIDES_DEPTH)
        assert np.array_equal(got[0], mine) and np.array_equal(got[2][..., 0] != np.float32(MISS_DEPTH), ids != capi.PT_INSTANCE_NONE)
        # the setter takes every bit pattern and the read-back returns it; None drops the plane
        words = np.random.default_rng(1).integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)
        r.set_instance_plane(words)
        assert np.array_equal(r.read_instance_plane(), words)
        r.set_instance_plane(None)
        with pytest.raises(capi.PtError) as e:
            r.read_instance_plane()
        assert e.value.code == capi.PT_ERR_STATE
        # a resize to the same size keeps the plane, one to another size drops it
        r.set_instance_plane(words)
        r.create((w, h))
        assert np.array_equal(r.read_instance_plane(), words)
        r.create((w + 3, h))
        with pytest.raises(capi.PtError) as e:
            r.read_instance_plane()
        assert e.value.code == capi.PT_ERR_STATE
        r.set_camera(host.camera_for(sc, w + 3, h, 0.0))
        r.render_instance_plane(0)
        assert r.read_instance_plane().shape == (h, w + 3)
    finally:
        r.destroy()


def test_errors():
    L = capi.lib()
    sc = gg.opaque_scene()
    w, h = SIZES[1]
    out = np.zeros((h, w), np.uint32)
    r = gg.open_renderer(None, (w, h))
    try:
        assert L.pt_render_instance_plane(r._ctx, 7, 1.0) == capi.PT_ERR_STATE and b"pt_build_accel" in L.pt_last_error(r._ctx)
        r.set_scene(sc)
        assert L.pt_render_instance_plane(r._ctx, 7, 1.0) == capi.PT_ERR_STATE and b"pt_set_camera" in L.pt_last_error(r._ctx)
    finally:
        r.destroy()
    r = gg.open_renderer(sc)
    try:
        r.set_camera(host.camera_for(sc, w, h, 0.0))
        for call in (lambda: L.pt_render_instance_plane(r._ctx, 0, 1.0), lambda: L.pt_read_instance_plane(r._ctx, out.ctypes.data), lambda: L.pt_set_instance_plane(r._ctx, out.ctypes.data)):
            assert call() == capi.PT_ERR_STATE and b"pt_resize" in L.pt_last_error(r._ctx)
        r.create((w, h))
        assert L.pt_read_instance_plane(r._ctx, out.ctypes.data) == capi.PT_ERR_STATE and b"instance plane" in L.pt_last_error(r._ctx)
        assert L.pt_read_instance_plane(r._ctx, None) == capi.PT_ERR_INVALID
        assert L.pt_render_instance_plane(None, 7, 1.0) == capi.PT_ERR_INVALID and L.pt_read_instance_plane(None, out.ctypes.data) == capi.PT_ERR_INVALID
        assert L.pt_set_instance_plane(None, out.ctypes.data) == capi.PT_ERR_INVALID
        r.render_instance_plane(7, MISS_DEPTH)
        ids, planes = r.read_instance_plane(), r.read_guides()
        # arguments: nothing is launched, the planes stay what they were (0 is no error here)
        for mask, miss in ((8, 1.0), (15, 1.0), (0x80000000, 1.0), (7, float("nan")), (0, float("inf")), (7, float("-inf"))):
            assert L.pt_render_instance_plane(r._ctx, mask, miss) == capi.PT_ERR_INVALID, (mask, miss)
        assert_ids_equal(r.read_instance_plane(), ids, "after refused calls")
        gg.assert_planes_equal(r.read_guides(), planes, "after refused calls")
    finally:
        r.destroy()


def test_an_overflow_of_its_walks_is_reported_by_the_next_synchronising_call():
    deep = Config(synth.deep_chain(synth.DEEP_OVERFLOW_LEVELS), gg.ENV, 32, 24, depth=2)
    r = gg.open_renderer(deep.scene, (32, 24))
    try:
        r.set_camera(deep.camera)
        r.render_instance_plane(0)
        with pytest.raises(capi.PtError) as e:
            r.read_instance_plane()
        assert e.value.code == capi.PT_ERR_STATE and "overflowed" in str(e.value)
        r.reset_stats()
        r.synchronize()
    finally:
        r.destroy()
