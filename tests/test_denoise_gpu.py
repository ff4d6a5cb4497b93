"""The denoiser on the device (pt_set_denoise_guides / pt_denoise / pt_tonemap_denoised through the C ABI) against the host build of the same header
(tests/denoise_host.py), which tests/test_denoise_model.py holds to the float64 model: device == host bit for bit on every pixel, non-finite ones
included, for both ways an iteration reads its taps (tile in LDS, straight from memory); the denoised display pass against pt_tonemap of the same image;
the calls leave rendering untouched; the stage lowers the error of a 1 spp frame; render_guides hands over what the existing entry points return."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from tests import denoise_host as dh
from tests.common import Config, render_hip
from vk_raytrace_amd import capi, host_device as hd, synth
from vk_raytrace_amd.renderer import HipRenderer, pixel_centre_rays
from vk_raytrace_amd.scene import Camera, Scene, rotate_y, translate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_denoise_kat", os.path.join(ROOT, "tests", "golden", "gen_denoise_kat.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

# not multiples of the 32 x 16 block tile, thinner than a halo (1 x 1, 3 x 200), smaller than step 16 (129 x 17 in y, 3 x 200 in x)
SIZES = [(70, 45), (1, 1), (3, 200), (129, 17)]
ITERATIONS = (1, 3, 5)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_inputs(w, h, seed):
    """HDR colour with about 3 % non-finite pixels (NaN, +-Inf, whole and per channel), an albedo with a step edge and values around the floor, a normal
    ramp, a depth plane with a step and a spike: any size"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    colour = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (h, w, 4))).astype(np.float32)
    bad = rng.uniform(size=(h, w, 3)) < 0.012
    colour[..., :3][bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
    albedo = np.zeros((h, w, 4), np.float32)
    albedo[..., :3] = np.where((xs < w // 2)[..., None], (0.8, 0.6, 0.4), (0.2, 0.3, 0.9))
    albedo[:max(1, h // 8), :max(1, w // 8), :3] = (0.0, 0.0005, 0.002)
    normal = np.zeros((h, w, 4), np.float32)
    normal[..., 0] = (xs / max(w - 1, 1)).astype(np.float32)
    normal[..., 1] = np.where(ys < h // 2, 0.0, 1.0)
    depth = np.zeros((h, w, 4), np.float32)
    depth[..., 0] = np.where(ys < h // 3, 3.0 + ys / max(h, 1), 6.0)
    depth[h // 2, w // 2, 0] = 56.0
    return colour, [albedo, normal, depth]


@pytest.fixture(scope="module")
def dev():
    r = HipRenderer()
    r.setup(0)
    yield r
    r.destroy()


def set_lds(r, max_step):
    return capi.lib().pt_debug_denoise_lds(r._ctx, max_step)


def compare_every_case(r, colour, guides, iterations, what):
    n = 0
    for installed in sorted({c[1] for c in gen.cases()}):
        planes = gen.case_guides(guides, installed)
        r.set_denoise_guides(*planes)
        for col, inst, flags in gen.cases():
            if inst != installed:
                continue
            for it in iterations:
                p = dh.params(it, gen.SIGMA_COLOR if col else 0.0, gen.SIGMA_GUIDE, flags)
                rc, want = dh.denoise(colour, planes, p)
                assert rc == 0
                got = r.denoise(p)
                diff = bits(got) != bits(want)
                assert not diff.any(), f"{what} colour={int(col)} guides={installed} flags={flags} x{it}: {int(diff.any(-1).sum())} pixels differ from the host build"
                n += 1
    return n


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_host_build_bit_for_bit(dev, size):
    """every case of the KAT: steps 1 and 2 from the LDS tile, steps 4 .. 16 from memory (the default), borders of both"""
    w, h = size
    colour, guides = make_inputs(w, h, 100 + w)
    dev.create((w, h))
    dev.write_accum(colour)
    assert set_lds(dev, -1) >= 0
    assert np.array_equal(bits(dev.read_accum()), bits(colour))
    assert compare_every_case(dev, colour, guides, ITERATIONS, f"{w}x{h}") == 24 * len(ITERATIONS)
    assert np.array_equal(bits(dev.read_accum()), bits(colour))   # the input is still what it was


@pytest.mark.parametrize("lds", [0, 1, 2])
def test_where_the_taps_are_read_from_changes_no_bit(dev, lds):
    """the same results with no iteration, only step 1, and steps 1 and 2 staged in LDS"""
    w, h = 70, 45
    colour, guides = make_inputs(w, h, 7)
    dev.create((w, h))
    dev.write_accum(colour)
    try:
        assert set_lds(dev, lds) == lds
        compare_every_case(dev, colour, guides, (3,), f"lds={lds}")
    finally:
        set_lds(dev, -1)


@pytest.mark.parametrize("auto_exposure", [0, 3])
def test_tonemap_denoised_is_tonemap_of_the_denoised_image(dev, auto_exposure):
    w, h = 70, 45
    colour, guides = make_inputs(w, h, 11)
    colour = np.where(np.isfinite(colour), colour, np.float32(1.0)).astype(np.float32)   # (a NaN would blank the auto-exposed image: nothing left to compare)
    dev.create((w, h))
    dev.write_accum(colour)
    dev.set_denoise_guides(*guides)
    tm = hd.default_tonemapper()
    tm.autoExposure = auto_exposure
    p = dh.params(3, gen.SIGMA_COLOR, gen.SIGMA_GUIDE, capi.PT_DENOISE_DEMODULATE)
    shown = dev.tonemap_denoised(p, tm)
    plain = dev.tonemap(tm)
    den = dev.denoise(p)
    dev.write_accum(den)
    want = dev.tonemap(tm)
    assert np.array_equal(shown, want)
    assert not np.array_equal(shown, plain)


def diffuse_scene():
    """a diffuse floor, a back wall and three tinted diffuse boxes under the environment: what the denoiser is for"""
    sc = Scene("denoise_diffuse")
    mats = [sc.add_material(pbrBaseColorFactor=c + (1,), pbrMetallicFactor=0.0, pbrRoughnessFactor=1.0)
            for c in ((0.7, 0.7, 0.7), (0.8, 0.25, 0.2), (0.2, 0.6, 0.3), (0.25, 0.3, 0.8), (0.6, 0.55, 0.4))]
    synth._add(sc, synth.grid(4, 4, (-3, 0, 3), (6, 0, 0), (0, 0, -6)), mats[0])
    synth._add(sc, synth.grid(4, 3, (-3, 0, -2), (6, 0, 0), (0, 3, 0)), mats[4])
    synth._add(sc, synth.box((0.8, 1.2, 0.8)), mats[1], translate(-1.0, 0.6, -0.6) @ rotate_y(0.5))
    synth._add(sc, synth.box((0.9, 0.7, 0.9)), mats[2], translate(0.4, 0.35, 0.2) @ rotate_y(-0.3))
    synth._add(sc, synth.box((0.5, 1.6, 0.5)), mats[3], translate(1.4, 0.8, -1.0) @ rotate_y(0.2))
    sc.camera = Camera(eye=(0.0, 1.6, 3.4), center=(0.0, 0.6, -0.5), up=(0, 1, 0), fov=50.0)
    return sc


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
    """frames 0 .. 2 with pt_denoise and pt_tonemap_denoised after frame 1: the accumulation image and the counters of pt_get_stats equal a run without them.
    The counters are compared with a run that synchronises where the calls do (how many rays the fused late-bounce kernel takes over follows the launch
    shapes, and three frames handed over at once are launched as one batch); the image also with a run that never stops."""
    cfg = Config(synth.feature_box(tex_size=32), synth.procedural_sky(64, 32), 64, 48)
    whole = render_hip(cfg, 3)
    p = dh.params(3, 1.0, (0.1, 0.3, 0.5))
    results = []
    for interrupt in (False, True):
        r, st = open_renderer(cfg)
        r.reset_stats()
        run_frames(r, st, (0, 1))
        if interrupt:
            planes = [np.full((48, 64, 4), v, np.float32) for v in (0.5, 0.25, 1.0)]
            r.set_denoise_guides(*planes)
            den = r.denoise(p)
            shown = r.tonemap_denoised(p, hd.default_tonemapper())
            assert np.isfinite(den).all() and shown.shape == (48, 64, 4)
        else:
            r.synchronize()
        run_frames(r, st, (2,))
        img = r.read_accum()
        stats = {k: v for k, v in r.stats().items() if not k.startswith("ms")}
        r.destroy()
        results.append((img, stats))
    (img_a, stats_a), (img_b, stats_b) = results
    assert np.array_equal(bits(img_a), bits(img_b)) and np.array_equal(bits(img_b), bits(whole))
    assert stats_a == stats_b and stats_a["samples"] == 3 * 64 * 48


def rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def test_it_denoises_and_the_guides_are_what_the_entry_points_return():
    """64 x 48, diffuse scene under a sky: guides from render_guides, 1 spp against the same scene at 256 spp.  The guide planes are the debug frames of
    eBaseColor and eNormal and the closest-hit distances of the pixel-centre rays, bit for bit."""
    w, h = 64, 48
    env = synth.procedural_sky(64, 32, sun_peak=50.0, sun_sigma_deg=10.0)
    cfg = Config(diffuse_scene(), env, w, h)
    r, st = open_renderer(cfg)
    try:
        albedo, normal, depth = r.render_guides(st)
        assert st.frame == 0 and st.debugging_mode == 0   # the caller's state is not modified
        for plane, mode in ((albedo, hd.eBaseColor), (normal, hd.eNormal)):
            direct = render_hip(Config(cfg.scene, env, w, h, debug=mode), 1)
            assert np.array_equal(bits(plane), bits(direct))
        hits = r.trace_rays(capi.PT_RAYS_CLOSEST, *pixel_centre_rays(cfg.camera, w, h))
        hit = (hits["status"] & capi.PT_RAY_HIT) != 0
        assert hit.sum() > w * h // 2 and (~hit).sum() > 0   # the scene fills most of the frame and leaves some sky
        assert np.array_equal(bits(depth[..., 0].reshape(-1)[hit]), bits(hits["t"][hit])) and (depth[..., 0].reshape(-1)[~hit] == np.float32(1e30)).all()
        assert (depth[..., 1:] == 0).all() and np.isfinite(albedo).all() and np.isfinite(normal).all()
        run_frames(r, st, (0,))
        noisy = r.read_accum()
        p = dh.params(4, 0.0, (0.1, 0.3, 0.3), capi.PT_DENOISE_DEMODULATE)
        den = r.denoise(p)
        rc, host = dh.denoise(noisy, [albedo, normal, depth], p)
        assert rc == 0 and np.array_equal(bits(den), bits(host))
        st.maxSamples = 256
        run_frames(r, st, (0,))
        target = r.read_accum()
    finally:
        r.destroy()
    e_noisy, e_den = rmse(noisy, target), rmse(den, target)
    print(f"RMSE against 256 spp: 1 spp {e_noisy:.5f}, denoised {e_den:.5f}")
    assert e_den < e_noisy


def test_errors():
    L = capi.lib()
    r = HipRenderer()
    r.setup(0)
    try:
        p, tm = dh.params(2, 1.0), hd.default_tonemapper()
        buf, rgba = np.zeros((45, 70, 4), np.float32), np.zeros((45, 70, 4), np.uint8)
        ptrs = (C.c_void_p * 3)(buf.ctypes.data, None, None)
        # before pt_resize
        assert L.pt_denoise(r._ctx, C.byref(p), buf.ctypes.data) == capi.PT_ERR_STATE
        assert L.pt_tonemap_denoised(r._ctx, C.byref(p), C.byref(tm), rgba.ctypes.data) == capi.PT_ERR_STATE
        assert L.pt_set_denoise_guides(r._ctx, ptrs) == capi.PT_ERR_STATE
        r.create((70, 45))
        r.write_accum(np.ones((45, 70, 4), np.float32))
        # arguments
        assert L.pt_denoise(r._ctx, None, buf.ctypes.data) == capi.PT_ERR_INVALID and L.pt_denoise(r._ctx, C.byref(p), None) == capi.PT_ERR_INVALID
        assert L.pt_tonemap_denoised(r._ctx, C.byref(p), None, rgba.ctypes.data) == capi.PT_ERR_INVALID
        assert L.pt_set_denoise_guides(r._ctx, None) == capi.PT_ERR_INVALID
        for bad in (dh.params(0, 1.0), dh.params(9, 1.0), dh.params(1, -1.0), dh.params(1, float("nan")), dh.params(1, 1.0, flags=2)):
            assert L.pt_denoise(r._ctx, C.byref(bad), buf.ctypes.data) == capi.PT_ERR_INVALID
        dem = dh.params(2, 1.0, flags=capi.PT_DENOISE_DEMODULATE)
        assert L.pt_denoise(r._ctx, C.byref(dem), buf.ctypes.data) == capi.PT_ERR_STATE   # no albedo plane
        r.set_denoise_guides(albedo=np.full((45, 70, 4), 0.5, np.float32))
        assert L.pt_denoise(r._ctx, C.byref(dem), buf.ctypes.data) == capi.PT_OK
        bad_sigma = dh.params(1, 1.0, (0.0, 1.0, 1.0))
        assert L.pt_denoise(r._ctx, C.byref(bad_sigma), buf.ctypes.data) == capi.PT_ERR_INVALID   # ... of an installed plane
        # pt_resize drops the guides
        r.create((64, 48))
        r.write_accum(np.ones((48, 64, 4), np.float32))
        small = np.zeros((48, 64, 4), np.float32)
        assert L.pt_denoise(r._ctx, C.byref(dem), small.ctypes.data) == capi.PT_ERR_STATE
        assert b"albedo" in L.pt_last_error(r._ctx)
        assert L.pt_denoise(r._ctx, C.byref(bad_sigma), small.ctypes.data) == capi.PT_OK          # no plane installed: its sigma is not read
    finally:
        r.destroy()
    # one of two ranks, nothing gathered
    r = HipRenderer()
    r.setup(0)
    try:
        r.set_shard(0, 2)
        r.create((70, 45))
        assert L.pt_denoise(r._ctx, C.byref(p), buf.ctypes.data) == capi.PT_ERR_STATE
        assert L.pt_tonemap_denoised(r._ctx, C.byref(p), C.byref(tm), rgba.ctypes.data) == capi.PT_ERR_STATE
    finally:
        r.destroy()
