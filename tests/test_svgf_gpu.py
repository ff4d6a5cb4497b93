"""The variance-guided filter on the device (pt_temporal_track_moments, pt_read_temporal_moments, pt_svgf_variance, pt_svgf_history, pt_tonemap_svgf
through the C ABI) against the host build of the same header (tests/svgf_host.py), which tests/test_svgf_model.py holds to the float64 model: device ==
host bit for bit on every pixel of the moments, the initial variance and the colour and variance after every iteration, non-finite pixels included, over
the camera moves of the fixture as three-call sequences; tracking changes nothing else; the LDS forms change no bit; the display bytes; the calls leave
rendering untouched; the state machine.  Sizes narrower and shorter than every halo and than the 7 x 7 window, and one column and one row past a tile."""
import ctypes as C

import numpy as np
import pytest

from tests import svgf_host as sh
from tests import test_svgf_model as model
from tests.common import Config, render_hip
from tests.test_temporal_gpu import camera_words, open_renderer, run_frames
from vk_raytrace_amd import capi, host_device as hd, synth
from vk_raytrace_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu
gen, bits = model.gen, model.bits

SIZES = [(70, 45), (45, 37), (1, 1), (3, 200), (129, 17)]
MOVES = [m for m in gen.MOVES if m != "first"]


@pytest.fixture(scope="module")
def dev():
    r = HipRenderer()
    r.setup(0)
    r.track_moments(True)
    yield r
    r.destroy()


def same(a, b, what):
    diff = bits(a) != bits(b)
    assert not diff.any(), f"{what}: {int(diff.sum())} words differ from the host build"


def sequence_inputs(size, move):
    """three calls: the start camera, the move, the moved camera again with other noise"""
    w, h = size
    first, second = gen.call_inputs(size, move, 0), gen.call_inputs(size, move, gen.STATIC_CALLS)
    third = dict(second, colour=gen.scene_colour(second["g1"], second["g2"], np.random.default_rng(5 * w + h)))
    return first, second, third


def step_both(r, hist, inp, what, compare=True):
    """one call with tracking on, on the device and on the host build from the host's history (which the device's has equalled so far)"""
    r.write_accum(inp["colour"])
    r.set_denoise_guides(inp["g0"], inp["g1"], inp["g2"])
    r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
    p = model.temporal_params(inp)
    got = r.temporal_accumulate(p)
    rc, want = sh.temporal_m(inp["colour"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], p, hist)
    assert rc == 0
    if compare:
        hc, hn = r.read_temporal_history()
        same(got, want.colour, f"{what}: returned image")
        same(hc, want.colour, f"{what}: history colour")
        same(hn, want.length, f"{what}: history length")
        same(r.read_temporal_moments(), want.moments, f"{what}: moments")
    return want


def filter_both(r, hist, guides, p, what, iterations=(1, 2, 3, 4, 5)):
    """V0 and the colour and variance after each count of iterations, device against host build"""
    rc, v0, steps = sh.filter_history(hist, guides, p)
    assert rc == 0
    same(r.svgf_variance(p), v0, f"{what}: V0")
    for n in iterations:
        q = hd.SvgfParams.from_buffer_copy(p)
        q.iterations = n
        c, v = r.svgf_history(q)
        same(c, steps[n - 1][0], f"{what}: colour after {n} iterations")
        same(v, steps[n - 1][1], f"{what}: variance after {n} iterations")
    return v0


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_host_build_bit_for_bit(dev, size):
    """every move as a three-call sequence, so that both buffer sets of the moments have been read and written; V0 after the first call (every pixel on the
    spatial branch), after the third with minTemporal 1 (every pixel with a history on the temporal branch) and with minTemporal 2.5 (mixed after a move that
    disoccludes); the filter after 1 .. 5 iterations"""
    w, h = size
    dev.create(size)
    for move in MOVES:
        dev.temporal_reset()
        hist = None
        for k, inp in enumerate(sequence_inputs(size, move)):
            hist = step_both(dev, hist, inp, f"{w}x{h} {move} call {k + 1}")
            guides = model.guides_of(inp)
            if k == 0:
                filter_both(dev, hist, guides, sh.params(5, min_temporal=3.5), f"{w}x{h} {move} spatial", iterations=(1,) if move != "yaw" else (1, 2, 3, 4, 5))
        filter_both(dev, hist, guides, sh.params(5, min_temporal=1.0), f"{w}x{h} {move} temporal", iterations=(2,))
        filter_both(dev, hist, guides, sh.params(5, min_temporal=2.5), f"{w}x{h} {move} mixed")
        if move == "disocclude" and w * h > 1000:
            long = hist.length >= 2.5
            assert 0.1 < long.mean() < 0.9          # both branches are taken


def test_tracking_changes_nothing_else():
    """the same sequence with tracking off and on: the returned image, the history colour and the length are the same bits; the setting survives pt_resize,
    a change of it drops the history, and only 0 and 1 are values"""
    L = capi.lib()
    size = (70, 45)
    runs = []
    for on in (False, True):
        r = HipRenderer()
        r.setup(0)
        try:
            r.track_moments(on)
            r.create((8, 8))
            r.create(size)          # the setting survives pt_resize
            out = []
            for inp in sequence_inputs(size, "yaw"):
                r.write_accum(inp["colour"])
                r.set_denoise_guides(None, inp["g1"], inp["g2"])
                r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
                out.append((r.temporal_accumulate(model.temporal_params(inp)),) + r.read_temporal_history())
            m = np.zeros(size[::-1] + (2,), np.float32)
            assert L.pt_read_temporal_moments(r._ctx, m.ctypes.data) == (capi.PT_OK if on else capi.PT_ERR_STATE)
            assert L.pt_temporal_track_moments(r._ctx, 2) == capi.PT_ERR_INVALID and L.pt_temporal_track_moments(r._ctx, -1) == capi.PT_ERR_INVALID
            r.track_moments(on)            # no change: the history stays
            r.read_temporal_history()
            r.track_moments(not on)        # a change drops it
            assert L.pt_read_temporal_history(r._ctx, m.ctypes.data, None) == capi.PT_ERR_STATE
            runs.append(out)
        finally:
            r.destroy()
    for k, (a, b) in enumerate(zip(*runs)):
        for x, y, name in zip(a, b, ("returned image", "history colour", "history length")):
            assert np.array_equal(bits(x), bits(y)), f"call {k + 1}: {name} depends on tracking"


@pytest.mark.parametrize("size", [(70, 45), (3, 200)], ids=["70x45", "3x200"])
def test_the_lds_forms_change_no_bit(dev, size):
    L = capi.lib()
    dev.create(size)
    dev.temporal_reset()
    hist = None
    for inp in sequence_inputs(size, "disocclude")[:2]:
        hist = step_both(dev, hist, inp, "lds", compare=False)
    p = sh.params(4, min_temporal=1.5)
    results = []
    try:
        for lds in (-1, 0, 1, 2):
            in_force = L.pt_debug_svgf_lds(dev._ctx, lds)
            assert in_force == lds if lds >= 0 else in_force in (0, 1, 2)
            results.append(dev.svgf_history(p))
    finally:
        L.pt_debug_svgf_lds(dev._ctx, -1)
    for c, v in results[1:]:
        assert np.array_equal(bits(c), bits(results[0][0])) and np.array_equal(bits(v), bits(results[0][1]))
    rc, _, steps = sh.filter_history(hist, model.guides_of(inp), p)
    same(results[0][0], steps[-1][0], "colour")


@pytest.mark.parametrize("planes", [(), (1,), (0, 1, 2)], ids=["no-plane", "one-plane", "three-planes"])
def test_guide_planes_installed_or_not(dev, planes):
    size = (45, 37)
    dev.create(size)
    dev.temporal_reset()
    hist = None
    for inp in sequence_inputs(size, "yaw")[:2]:
        hist = step_both(dev, hist, inp, "planes", compare=False)
    guides = model.guides_of(inp, planes)
    dev.set_denoise_guides(*guides)
    # sigmaGuide of a plane that is not installed is not read: hostile there
    sigma = tuple(0.4 if j in planes else np.nan for j in range(3))
    filter_both(dev, hist, guides, sh.params(5, sigma_guide=sigma, min_temporal=1.5), f"planes {planes}", iterations=(1, 3))


@pytest.mark.parametrize("auto_exposure", [0, 3])
def test_the_display_of_the_filtered_history(dev, auto_exposure):
    """pt_tonemap_svgf is pt_tonemap after pt_write_accum(pt_svgf_history's image)"""
    size = (70, 45)
    dev.create(size)
    dev.temporal_reset()
    hist = None
    for inp in sequence_inputs(size, "strafe")[:2]:
        inp = dict(inp, colour=np.where(np.isfinite(inp["colour"]), inp["colour"], np.float32(1.0)).astype(np.float32))   # (a NaN would blank the auto-exposed image)
        hist = step_both(dev, hist, inp, "display", compare=False)
    tm = hd.default_tonemapper()
    tm.autoExposure = auto_exposure
    p = sh.params(3, min_temporal=1.5)
    shown, (filtered, _) = dev.tonemap_svgf(p, tm), dev.svgf_history(p)
    hc, hn = dev.read_temporal_history()
    same(hc, hist.colour, "the history after the calls")          # they only read it
    same(dev.read_temporal_moments(), hist.moments, "the moments after the calls")
    dev.write_accum(filtered)
    assert np.array_equal(shown, dev.tonemap(tm))
    dev.write_accum(hc)
    assert not np.array_equal(shown, dev.tonemap(tm))


def test_the_calls_leave_rendering_untouched():
    """frames 0 .. 1, the guide pass, then tracking on, pt_temporal_accumulate (twice), pt_svgf_variance, pt_svgf_history and pt_tonemap_svgf, then frame 2: the
    accumulation image, the counters of pt_get_stats and the guide planes equal a run that only synchronises there"""
    cfg = Config(synth.feature_box(tex_size=32), synth.procedural_sky(64, 32), 64, 48)
    whole = render_hip(cfg, 3)
    tm = hd.default_tonemapper()
    results = []
    for interrupt in (False, True):
        r, st = open_renderer(cfg)
        r.reset_stats()
        run_frames(r, st, (0, 1))
        r.capture_guides(7, 50.0)
        planes = r.read_guides()
        if interrupt:
            r.track_moments(True)
            p = r.temporal_params(r.world_to_clip(cfg.scene.camera, 64 / 48))
            r.temporal_accumulate(p)
            r.temporal_accumulate(p)
            sp = r.svgf_params(4, min_temporal=1.5)
            filtered, var = r.svgf_history(sp)
            assert np.isfinite(filtered).all() and np.isfinite(var).all() and (r.svgf_variance(sp) >= 0).all() and r.tonemap_svgf(sp, tm).shape == (48, 64, 4)
            assert np.isfinite(r.read_temporal_moments()).all()
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(planes, r.read_guides()))
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


def test_errors_launch_nothing():
    L = capi.lib()
    size = (45, 37)
    w, h = size
    first, second, _ = sequence_inputs(size, "strafe")
    good, tm = sh.params(3, min_temporal=1.5), hd.default_tonemapper()
    out, var, rgba, m = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 2), np.float32)
    r = HipRenderer()
    r.setup(0)
    try:
        def calls(p):
            q = None if p is None else C.byref(p)
            return (L.pt_svgf_variance(r._ctx, q, var.ctypes.data), L.pt_svgf_history(r._ctx, q, out.ctypes.data, var.ctypes.data),
                    L.pt_svgf_history(r._ctx, q, out.ctypes.data, None), L.pt_tonemap_svgf(r._ctx, q, C.byref(tm), rgba.ctypes.data))
        # before pt_resize
        assert calls(good) == (capi.PT_ERR_STATE,) * 4 and b"pt_resize" in L.pt_last_error(r._ctx)
        assert L.pt_read_temporal_moments(r._ctx, m.ctypes.data) == capi.PT_ERR_STATE
        assert L.pt_temporal_track_moments(None, 1) == capi.PT_ERR_INVALID and L.pt_svgf_history(None, C.byref(good), out.ctypes.data, None) == capi.PT_ERR_INVALID
        r.create(size)
        # without a history
        assert calls(good) == (capi.PT_ERR_STATE,) * 4 and b"no history" in L.pt_last_error(r._ctx)
        # with a history made while tracking was off
        r.write_accum(first["colour"])
        r.set_denoise_guides(first["g0"], first["g1"], first["g2"])
        r.set_camera(camera_words((first["viewInverse"], first["projInverse"])))
        r.temporal_accumulate(model.temporal_params(first))
        assert calls(good) == (capi.PT_ERR_STATE,) * 4 and b"without moments" in L.pt_last_error(r._ctx)
        assert L.pt_read_temporal_moments(r._ctx, m.ctypes.data) == capi.PT_ERR_STATE
        r.track_moments(True)
        assert calls(good) == (capi.PT_ERR_STATE,) * 4 and b"no history" in L.pt_last_error(r._ctx)
        r.temporal_accumulate(model.temporal_params(first))
        assert calls(good) == (capi.PT_OK,) * 4
        before = (out.copy(), var.copy())
        # PT_ERR_INVALID per svgf_constants, nothing launched: the outputs stay as they were
        bad = [None] + [sh.params(i) for i in (0, 9)] + [sh.params(2, sigma_lum=x) for x in (0.0, np.nan, np.inf)] + [sh.params(2, lum_floor=x) for x in (0.0, -1.0, np.inf)]
        bad += [sh.params(2, min_temporal=x) for x in (0.5, np.nan)] + [sh.params(2, sigma_guide=(1.0, 0.0, 1.0)), sh.params(2, sigma_guide=(1e-30, 1.0, 1.0)), sh.params(2, flags=1)]
        for p in bad:
            assert calls(p) == (capi.PT_ERR_INVALID,) * 4
            assert np.array_equal(bits(out), bits(before[0])) and np.array_equal(bits(var), bits(before[1]))
        assert L.pt_svgf_variance(r._ctx, C.byref(good), None) == capi.PT_ERR_INVALID and L.pt_svgf_history(r._ctx, C.byref(good), None, None) == capi.PT_ERR_INVALID
        assert L.pt_tonemap_svgf(r._ctx, C.byref(good), None, rgba.ctypes.data) == capi.PT_ERR_INVALID and L.pt_read_temporal_moments(r._ctx, None) == capi.PT_ERR_INVALID
        # pt_temporal_reset and pt_resize drop the history, moments included
        r.temporal_reset()
        assert calls(good) == (capi.PT_ERR_STATE,) * 4 and L.pt_read_temporal_moments(r._ctx, m.ctypes.data) == capi.PT_ERR_STATE
        r.temporal_accumulate(model.temporal_params(first))
        assert calls(good) == (capi.PT_OK,) * 4
        r.create((64, 48))
        assert calls(good) == (capi.PT_ERR_STATE,) * 4
    finally:
        r.destroy()
