"""The temporal stage on the device (pt_temporal_accumulate and its companions through the C ABI) against the host build of the same header
(tests/temporal_host.py), which tests/test_temporal_model.py holds to the float64 model: device == host bit for bit on every pixel of the history
colour, the length plane and the returned image, non-finite pixels included, over every camera move of the fixture, hostile matrices and depths, and
three-call sequences that read and write both buffer sets; a rendered sequence; the calls leave rendering untouched; the display of the history; the
state machine."""
import ctypes as C

import numpy as np
import pytest

from tests import denoise_host as dh, path_kat_io, temporal_host as th
from tests import test_temporal_model as model
from tests.common import Config, render_hip
from vk_raytrace_amd import capi, host_device as hd, synth
from vk_raytrace_amd.renderer import HipRenderer
from vk_raytrace_amd.scene import Camera

pytestmark = pytest.mark.gpu
gen, bits = model.gen, model.bits

# not multiples of the 32 x 8 block tile, one pixel, thinner than a tile in each direction
SIZES = [(70, 45), (45, 37), (1, 1), (3, 200), (129, 17)]
MOVES = [m for m in gen.MOVES if m != "first"]


@pytest.fixture(scope="module")
def dev():
    r = HipRenderer()
    r.setup(0)
    yield r
    r.destroy()


def scene_camera(view_inverse, proj_inverse):
    cam = hd.SceneCamera()
    cam.viewInverse[:], cam.projInverse[:] = [float(x) for x in view_inverse], [float(x) for x in proj_inverse]
    return cam


def camera_words(cam):
    """SceneCamera with the words given, bit for bit (hostile values included)"""
    out = hd.SceneCamera()
    C.memmove(out.viewInverse, np.ascontiguousarray(cam[0], np.float32).ctypes.data, 64)
    C.memmove(out.projInverse, np.ascontiguousarray(cam[1], np.float32).ctypes.data, 64)
    return out


def step_both(r, hist, colour, g1, g2, view_inverse, proj_inverse, p, what):
    """one call on the device and on the host build, from the same inputs and the host's history (which the device's has equalled so far); compares
    everything the device hands out and returns the host's new history"""
    r.write_accum(colour)
    r.set_denoise_guides(None, g1, g2)
    r.set_camera(camera_words((view_inverse, proj_inverse)))
    got = r.temporal_accumulate(p)
    hc, hn = r.read_temporal_history()
    rc, want = th.temporal(colour, g1, g2, view_inverse, proj_inverse, p, hist)
    assert rc == 0
    for name, a, b in (("returned image", got, want.colour), ("history colour", hc, want.colour), ("history length", hn, want.length)):
        diff = bits(a) != bits(b)
        assert not diff.any(), f"{what}: {name} differs from the host build at {int(diff.reshape(diff.shape[0], diff.shape[1], -1).any(-1).sum())} pixels"
    return want


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_host_build_bit_for_bit(dev, size):
    """every move of the fixture as a three-call sequence -- a first call at the start camera, the move, a static call after it -- so that both buffer
    sets have been read and written; then hostile forward matrices, depths and cameras"""
    w, h = size
    dev.create((w, h))
    for move in MOVES:
        dev.temporal_reset()
        inp = gen.case_inputs(size, move)
        H = inp["hist"]
        start = gen.moved("none", w / h)
        g1_0, g2_0 = gen.guides(start, w, h)
        p0 = th.params(start["worldToClip"], gen.DEPTH_TOL, gen.NORMAL_DIST2, gen.MAX_HISTORY)
        hist = step_both(dev, None, H["colour"], g1_0, g2_0, start["viewInverse"], start["projInverse"], p0, f"{w}x{h} {move} call 1")
        p = model.params_of(inp)
        hist = step_both(dev, hist, inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], p, f"{w}x{h} {move} call 2")
        again = gen.noisy_colour(w, h, np.random.default_rng(w + h))
        step_both(dev, hist, again, inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], p, f"{w}x{h} {move} call 3")
    rng = np.random.default_rng(w * 7 + h)
    for k in range(6):
        dev.temporal_reset()
        inp = model.adversarial(rng, w, h)
        H = inp["hist"]
        w2c = np.where(np.isfinite(H["worldToClip"]), H["worldToClip"], np.float32(3.0e38)).astype(np.float32)   # (the entry point refuses what is not finite)
        start = gen.moved("none", w / h)
        g1_0, g2_0 = gen.guides(start, w, h)
        p0 = th.params(w2c, gen.DEPTH_TOL, gen.NORMAL_DIST2, gen.MAX_HISTORY)
        hist = step_both(dev, None, H["colour"], g1_0, g2_0, start["viewInverse"], start["projInverse"], p0, f"{w}x{h} hostile {k} call 1")
        p = th.params(inp["worldToClip"], 1.0e30 if k % 2 else gen.DEPTH_TOL, gen.NORMAL_DIST2, gen.MAX_HISTORY)
        hist = step_both(dev, hist, inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], p, f"{w}x{h} hostile {k} call 2")
        step_both(dev, hist, inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], p, f"{w}x{h} hostile {k} call 3")


# ---- a rendered sequence ----------------------------------------------------------------------------------------------------------------------------------
def box_config(kat):
    """the 32-triangle box of the path fixture at 96 x 64, its first configuration"""
    cfg = path_kat_io.config(kat, str(kat["config_names"][0]))
    cfg.width, cfg.height = 96, 64
    return cfg


def box_camera(k, aspect):
    """three cameras a fraction of a pixel and a fraction of a degree apart, around the fixture's own"""
    eye = np.array([0.1, 0.1, 1.7]) + k * np.array([0.004, 0.0, 0.0])
    center = np.array([-0.1, -0.25, -2.0]) + k * np.array([0.01, 0.002, 0.0])
    return Camera(eye=tuple(eye), center=tuple(center), up=(0, 1, 0), fov=70.0)


def rmse(a, b, sel):
    d = a[..., :3][sel].astype(np.float64) - b[..., :3][sel].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL], ids=["flat", "two-level"])
def test_a_rendered_sequence(accel):
    """three rounds of camera, pt_render_guides, frame 0, pt_temporal_accumulate: the host build, fed the images and planes read back, reproduces history
    and lengths bit for bit; and over the three moves (RtxState offers no seed besides the frame number) the history of the pixels that kept theirs
    throughout is closer to a 256 spp image of the last camera than the last 1 spp frame alone -- a sanity inequality, no threshold on the gain"""
    kat = path_kat_io.load()
    cfg = box_config(kat)
    w, h = cfg.width, cfg.height
    r = HipRenderer()
    r.setup(0)
    try:
        r.set_accel_mode(accel)
        r.set_scene(cfg.scene)
        integral, _ = r.set_env(cfg.env)
        r.set_sunsky(cfg.sunsky)
        r.create((w, h))
        st = cfg.state(integral)
        hist = None
        for k in range(3):
            cam_k = box_camera(k, w / h)
            cam = capi.camera_lookat(cam_k, w / h, nb_lights=len(cfg.scene.lights))
            r.set_camera(cam)
            r.capture_guides(7, 50.0)
            st.frame = 0
            r.setPushContants(st)
            r.run()
            frame = r.read_accum()
            _, g1, g2 = r.read_guides(6)
            p = r.temporal_params(r.world_to_clip(cam_k, w / h), 0.05, 0.05, 16.0)
            got = r.temporal_accumulate(p)
            hc, hn = r.read_temporal_history()
            rc, hist = th.temporal(frame, g1, g2, np.array(cam.viewInverse, np.float32), np.array(cam.projInverse, np.float32), p, hist)
            assert rc == 0
            assert np.array_equal(bits(got), bits(hist.colour)) and np.array_equal(bits(hc), bits(hist.colour)) and np.array_equal(bits(hn), bits(hist.length)), k
        st.maxSamples = 256
        r.setPushContants(st)
        r.run()
        target = r.read_accum()
    finally:
        r.destroy()
    # (the fixture's materials leave a few pixels of a 1 spp frame without a finite colour: an RMS error exists where all three images are finite)
    old = (hn >= 3) & gen.finite3(frame) & gen.finite3(hc) & gen.finite3(target)
    assert old.sum() > 0.3 * w * h, int(old.sum())
    e_frame, e_hist = rmse(frame, target, old), rmse(hc, target, old)
    print(f"RMSE against 256 spp on {int(old.sum())} pixels of length >= 3: last 1 spp frame {e_frame:.5f}, history {e_hist:.5f}")
    assert e_hist < e_frame


# ---- rendering untouched ------------------------------------------------------------------------------------------------------------------------------------
def open_renderer(cfg):
    r = HipRenderer()
    r.setup(0)
    r.set_scene(cfg.scene)
    integral, _ = r.set_env(cfg.env)
    r.set_camera(cfg.camera)
    r.set_sunsky(cfg.sunsky)
    r.create((cfg.width, cfg.height))
    return r, cfg.state(integral)


def run_frames(r, st, frames):
    for f in frames:
        st.frame = f
        r.setPushContants(st)
        r.run()


def test_the_calls_leave_rendering_untouched():
    """frames 0 .. 1, the guide pass, then pt_temporal_accumulate (twice), pt_denoise_history and pt_tonemap_history, then frame 2: the accumulation image, the
    counters of pt_get_stats and the guide planes equal a run that only synchronises there; pt_denoise and pt_tonemap_denoised return the same bytes with
    and without a history present"""
    cfg = Config(synth.feature_box(tex_size=32), synth.procedural_sky(64, 32), 64, 48)
    whole = render_hip(cfg, 3)
    dp, tm = dh.params(3, 1.0, (0.1, 0.3, 0.5)), hd.default_tonemapper()
    results = []
    for interrupt in (False, True):
        r, st = open_renderer(cfg)
        r.reset_stats()
        run_frames(r, st, (0, 1))
        r.capture_guides(7, 50.0)
        planes = r.read_guides()
        if interrupt:
            p = r.temporal_params(r.world_to_clip(cfg.scene.camera, 64 / 48))
            first = r.temporal_accumulate(p)
            assert np.array_equal(bits(first), bits(r.read_accum()))      # no history yet: the accumulation image itself
            second = r.temporal_accumulate(p)
            assert np.isfinite(second).all() and np.isfinite(r.denoise_history(dp)).all() and r.tonemap_history(dp, tm).shape == (48, 64, 4)
            after = r.read_guides()
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(planes, after))
        else:
            r.synchronize()
        shown = (r.denoise(dp), r.tonemap_denoised(dp, tm))
        run_frames(r, st, (2,))
        img = r.read_accum()
        stats = {k: v for k, v in r.stats().items() if not k.startswith("ms")}
        r.destroy()
        results.append((img, stats, shown))
    (img_a, stats_a, shown_a), (img_b, stats_b, shown_b) = results
    assert np.array_equal(bits(img_a), bits(img_b)) and np.array_equal(bits(img_b), bits(whole))
    assert stats_a == stats_b and stats_a["samples"] == 3 * 64 * 48
    assert np.array_equal(bits(shown_a[0]), bits(shown_b[0])) and np.array_equal(shown_a[1], shown_b[1])


# ---- display bytes ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto_exposure", [0, 3])
def test_the_display_of_the_history(dev, auto_exposure):
    """pt_tonemap_history(NULL) is pt_tonemap after pt_write_accum(Hc); pt_tonemap_history(dp) is pt_tonemap after pt_write_accum(pt_denoise_history(dp))"""
    size = (70, 45)
    w, h = size
    dev.create(size)
    dev.temporal_reset()
    hist = None
    for move in ("none", "strafe"):
        inp = gen.case_inputs(size, move)
        colour = np.where(np.isfinite(inp["colour"]), inp["colour"], np.float32(1.0)).astype(np.float32)   # (a NaN would blank the auto-exposed image: nothing left to compare)
        hist = step_both(dev, hist, colour, inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], model.params_of(inp), move)
    tm = hd.default_tonemapper()
    tm.autoExposure = auto_exposure
    dp = dh.params(3, gen.DEPTH_TOL * 50, (1.0, 0.3, 0.5))
    plain, filtered, den = dev.tonemap_history(None, tm), dev.tonemap_history(dp, tm), dev.denoise_history(dp)
    hc, hn = dev.read_temporal_history()
    assert np.array_equal(bits(hc), bits(hist.colour)) and np.array_equal(bits(hn), bits(hist.length))      # both calls only read the history
    rc, want = dh.denoise(hc, [None, inp["g1"], inp["g2"]], dp)
    assert rc == 0 and np.array_equal(bits(den), bits(want))
    dev.write_accum(hc)
    assert np.array_equal(plain, dev.tonemap(tm))
    dev.write_accum(den)
    assert np.array_equal(filtered, dev.tonemap(tm))
    assert not np.array_equal(plain, filtered)


# ---- the state machine --------------------------------------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing_and_leave_the_history_alone():
    L = capi.lib()
    size = (45, 37)
    w, h = size
    inp = gen.case_inputs(size, "strafe")
    good = model.params_of(inp)
    out = np.zeros((h, w, 4), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    dp, tm = dh.params(2, 1.0), hd.default_tonemapper()
    r = HipRenderer()
    r.setup(0)
    try:
        def call(p):
            return L.pt_temporal_accumulate(r._ctx, None if p is None else C.byref(p), out.ctypes.data)
        # before pt_resize, before pt_set_camera, without the planes
        assert call(good) == capi.PT_ERR_STATE and b"pt_resize" in L.pt_last_error(r._ctx)
        assert L.pt_read_temporal_history(r._ctx, out.ctypes.data, None) == capi.PT_ERR_STATE
        assert L.pt_denoise_history(r._ctx, C.byref(dp), out.ctypes.data) == capi.PT_ERR_STATE
        assert L.pt_tonemap_history(r._ctx, None, C.byref(tm), rgba.ctypes.data) == capi.PT_ERR_STATE
        assert L.pt_temporal_reset(r._ctx) == capi.PT_OK and L.pt_temporal_reset(None) == capi.PT_ERR_INVALID
        r.create(size)
        r.write_accum(inp["colour"])
        assert call(good) == capi.PT_ERR_STATE and b"pt_set_camera" in L.pt_last_error(r._ctx)
        r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
        assert call(good) == capi.PT_ERR_STATE and b"guide planes" in L.pt_last_error(r._ctx)
        r.set_denoise_guides(None, inp["g1"], None)
        assert call(good) == capi.PT_ERR_STATE
        r.set_denoise_guides(None, inp["g1"], inp["g2"])
        assert L.pt_read_temporal_history(r._ctx, out.ctypes.data, None) == capi.PT_ERR_STATE     # none of that made a history
        assert call(good) == capi.PT_OK
        assert L.pt_temporal_accumulate(r._ctx, C.byref(good), None) == capi.PT_OK                  # the image is optional
        before = r.read_temporal_history()
        # PT_ERR_INVALID: nothing launched, the history untouched
        eye = np.array(good.worldToClip, np.float32)
        bad = [None]
        for i, v in ((0, np.nan), (15, np.inf), (7, -np.inf)):
            m = eye.copy()
            m[i] = v
            bad.append(th.params(m, gen.DEPTH_TOL, gen.NORMAL_DIST2, gen.MAX_HISTORY))
        bad += [th.params(eye, v, gen.NORMAL_DIST2, gen.MAX_HISTORY) for v in (0.0, -1.0, np.nan, np.inf)]
        bad += [th.params(eye, gen.DEPTH_TOL, v, gen.MAX_HISTORY) for v in (-1.0, np.nan, np.inf)]
        bad += [th.params(eye, gen.DEPTH_TOL, gen.NORMAL_DIST2, v) for v in (0.5, np.nan, np.inf)]
        bad += [th.params(eye, gen.DEPTH_TOL, gen.NORMAL_DIST2, gen.MAX_HISTORY, flags=f) for f in (1, 4)]
        for p in bad:
            assert call(p) == capi.PT_ERR_INVALID
            after = r.read_temporal_history()
            assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))
        assert L.pt_denoise_history(r._ctx, None, out.ctypes.data) == capi.PT_ERR_INVALID and L.pt_denoise_history(r._ctx, C.byref(dp), None) == capi.PT_ERR_INVALID
        assert L.pt_denoise_history(r._ctx, C.byref(dh.params(0, 1.0)), out.ctypes.data) == capi.PT_ERR_INVALID
        assert L.pt_tonemap_history(r._ctx, None, None, rgba.ctypes.data) == capi.PT_ERR_INVALID
        assert L.pt_read_temporal_history(r._ctx, None, None) == capi.PT_OK
        # a state error with a history present leaves it alone too
        r.set_denoise_guides(None, inp["g1"], None)
        assert call(good) == capi.PT_ERR_STATE
        after = r.read_temporal_history()
        assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))
        r.set_denoise_guides(None, inp["g1"], inp["g2"])
        # pt_temporal_reset drops it: the next call is a first call
        r.temporal_reset()
        assert L.pt_read_temporal_history(r._ctx, out.ctypes.data, None) == capi.PT_ERR_STATE
        got = r.temporal_accumulate(good)
        _, hn = r.read_temporal_history()
        assert np.array_equal(bits(got), bits(inp["colour"])) and np.array_equal(hn, np.where(gen.finite3(inp["colour"]), 1.0, 0.0).astype(np.float32))
        # ... and so does pt_resize
        r.create((64, 48))
        assert L.pt_read_temporal_history(r._ctx, out.ctypes.data, None) == capi.PT_ERR_STATE
        small = gen.case_inputs((64, 48), "strafe")
        r.write_accum(small["colour"])
        r.set_denoise_guides(None, small["g1"], small["g2"])
        got = r.temporal_accumulate(model.params_of(small))
        assert np.array_equal(bits(got), bits(small["colour"]))
    finally:
        r.destroy()
    # one of two ranks, nothing gathered
    r = HipRenderer()
    r.setup(0)
    try:
        r.set_shard(0, 2)
        r.create(size)
        r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
        r.set_denoise_guides(None, inp["g1"], inp["g2"])
        assert L.pt_temporal_accumulate(r._ctx, C.byref(good), out.ctypes.data) == capi.PT_ERR_STATE and b"gather" in L.pt_last_error(r._ctx)
    finally:
        r.destroy()


def test_a_pending_traversal_stack_overflow_is_reported():
    """frames of the scene that is deeper than the traversal stack (tests/test_gpu_edges.py pins the contract): the stage says so like every call that
    hands out results"""
    env = synth.procedural_sky(64, 32)
    deep = Config(synth.deep_chain(synth.DEEP_OVERFLOW_LEVELS), env, 32, 24, depth=2)
    r, st = open_renderer(deep)
    try:
        planes = [np.full((24, 32, 4), v, np.float32) for v in (0.5, 3.0)]
        r.set_denoise_guides(None, *planes)
        run_frames(r, st, (0,))
        p = r.temporal_params(r.world_to_clip(deep.scene.camera, 32 / 24))
        with pytest.raises(capi.PtError) as e:
            r.temporal_accumulate(p)
        assert e.value.code == capi.PT_ERR_STATE and "overflowed" in str(e.value)
    finally:
        r.destroy()
