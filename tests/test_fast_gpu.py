"""The responsive history on the device (pt_temporal_fast) against the host build of the same headers (tests/fast_host.py), which
tests/test_fast_model.py holds to the parent's host builds and to the float64 model: device == host bit for bit on every pixel of the returned image, the
clamped history colour, the lowered length, the fast colour and the fast length (and, with tracking on, the moments), for radius 1, 2 and 3 over a first
call, a static call and the move; the moving form; all four combinations of tracking and demodulation; hostile planes; through the consumers; the setting
off changes no byte; the refusals leave the histories untouched; the state the context keeps; the timing entry."""
import ctypes as C

import numpy as np
import pytest

from tests import albedo_host as ah, fast_host as fh, motion_host as mh, svgf_host as sh
from tests import test_fast_model as model
from tests.test_motion_gpu import identity_worlds, node_array, three_node_scene, words_of
from tests.test_temporal_gpu import camera_words
from vk_raytrace_amd import capi, host_device as hd
from vk_raytrace_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu
fk, ak, sk, mk, tk, bits = model.fk, model.ak, model.sk, model.mk, model.tk, model.bits

# tile edges of the 32 x 16 block, a lone pixel (n < 2), a column narrower than the halo, a one-column tile and a tile with one row past 16
SIZES = [(70, 45), (45, 37), (1, 1), (3, 200), (129, 17)]


@pytest.fixture(scope="module")
def dev():
    r = HipRenderer()
    r.setup(0)
    sc = three_node_scene()
    r.set_scene(sc)
    yield r, sc
    r.temporal_fast(None)
    r.temporal_demodulate(False)
    r.track_moments(False)
    r.destroy()


def same(a, b, what):
    diff = bits(a) != bits(b)
    assert not diff.any(), f"{what}: {int(diff.sum())} words differ from the host build"


def step_both(r, hist, inp, fp, what, moments=False, demod=False, ids=None, tab=None):
    """one call with the setting on, on the device and on the host build from the host's history (which the device's has equalled so far); ids: the moving
    form, with the table the host build takes"""
    r.write_accum(inp["colour"])
    r.set_denoise_guides(inp["g0"], inp["g1"], inp["g2"])
    r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
    p = model.params_of(inp)
    if ids is None:
        got = r.temporal_accumulate(p)
    else:
        r.set_instance_plane(ids)
        got = r.temporal_accumulate_moving(p)
    rc, want = fh.step(inp["colour"], inp["g0"] if demod else None, inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], p, fp, hist, moments=moments, ids=ids, tab=tab)
    assert rc == 0
    hc, hn = r.read_temporal_history()
    hf, hnf = r.read_temporal_fast()
    same(got, want.colour, f"{what}: returned image")
    same(hc, want.colour, f"{what}: clamped history colour")
    same(hn, want.length, f"{what}: lowered history length")
    same(hf, want.fast, f"{what}: fast colour")
    same(hnf, want.fast_length, f"{what}: fast length")
    if moments:
        same(r.read_temporal_moments(), want.moments, f"{what}: moments")
    return want


def clamped_pixels(hist):
    return int((bits(hist.colour) != bits(hist.raw)).any(-1).sum())


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_host_build_bit_for_bit(dev, size, radius):
    """the static form: a first call, a static call and the move"""
    r, _ = dev
    w, h = size
    r.create(size)
    r.track_moments(False)
    r.temporal_demodulate(False)
    fp = fh.params(2.5, 1.0, radius)
    r.temporal_fast(fp)
    r.temporal_reset()
    hist, moved = None, 0
    for k in (0, 1, sk.STATIC_CALLS):
        hist = step_both(r, hist, sk.call_inputs(size, "yaw", k), fp, f"{w}x{h} radius {radius} call {k}")
        moved += clamped_pixels(hist)
    assert moved > 0 or w * h == 1


@pytest.mark.parametrize("demod", [False, True], ids=["raw", "demodulated"])
@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
def test_every_combination_of_the_settings(dev, moments, demod):
    """45 x 37, tracking and demodulation on and off: five calls of the sequence, then the consumers of what that leaves"""
    r, _ = dev
    size = (45, 37)
    r.create(size)
    r.track_moments(moments)
    r.temporal_demodulate(demod)
    fp = model.fast_params()
    r.temporal_fast(fp)
    r.temporal_reset()
    hist = None
    for k in range(sk.calls_of("disocclude")):
        inp = model.inputs_of(size, "disocclude", k, demod)
        hist = step_both(r, hist, inp, fp, f"call {k} moments {moments} demodulated {demod}", moments, demod)
    assert clamped_pixels(hist) > 100 and (hist.length < hist.raw_length).sum() > 20
    if moments:
        consumers_both(r, hist, inp, demod, f"moments {moments} demodulated {demod}")


def consumers_both(r, hist, inp, demod, what):
    """pt_svgf_variance, pt_svgf_history and pt_tonemap_svgf after a clamped step against the host builds fed the clamped history (colour, lowered length and
    the untouched moments); the display bytes against pt_tonemap of the float result"""
    guides = (inp["g0"], inp["g1"], inp["g2"])
    tm = hd.default_tonemapper()
    sp = sh.params(3, sigma_guide=(1e15, 0.3, 0.5), min_temporal=2.5)     # (lengths the clamp lowered to maxFast fall below it: the spatial estimate)
    host_hist = sh.History(hist.colour, hist.guide, hist.length, hist.moments, hist.world_to_clip, hist.eye)
    rc, v0 = sh.variance(hist.colour, hist.length, hist.moments, guides, sp)
    assert rc == 0
    same(r.svgf_variance(sp), v0, f"{what}: V0 of the clamped history")
    if demod:
        rc, img, var = ah.svgf_history(hist, guides, sp)
    else:
        rc, _, steps = sh.filter_history(host_hist, guides, sp)
        img, var = steps[-1]
    assert rc == 0
    c, v = r.svgf_history(sp)
    same(c, img, f"{what}: pt_svgf_history")
    same(v, var, f"{what}: variance")
    shown = r.tonemap_svgf(sp, tm)
    r.write_accum(c)
    assert np.array_equal(shown, r.tonemap(tm)), f"{what}: pt_tonemap_svgf"


def test_the_moving_form_equals_the_host_build_bit_for_bit(dev):
    """70 x 45, one moved instance: a first call with the box where the history has it, pt_update_instances and the move, a call after it"""
    r, sc = dev
    size = (70, 45)
    w, h = size
    r.create(size)
    r.track_moments(False)
    r.temporal_demodulate(False)
    fp = model.fast_params()
    r.temporal_fast(fp)
    r.temporal_reset()
    inp = mk.case_inputs(size, "slide")
    inp["g0"] = None
    H = inp["hist"]
    start = tk.moved("none", w / h)
    g2_0 = np.zeros((h, w, 4), np.float32)
    g1_0 = H["guide"].copy()
    g1_0[..., 3], g2_0[..., 0] = 1.0, H["guide"][..., 3]
    first = dict(inp, colour=H["colour"], g1=g1_0, g2=g2_0, viewInverse=start["viewInverse"], projInverse=start["projInverse"], worldToClip=start["worldToClip"])
    r.update_instances(node_array(sc, identity_worlds()))
    hist = step_both(r, None, first, fp, "moving call 1", ids=H["ids"])
    words = words_of(identity_worlds())
    worlds = identity_worlds(inp["box"])
    r.update_instances(node_array(sc, worlds))
    tab = mh.table(words, words_of(worlds))
    assert mh.moved_bits(tab).tolist() == [0, 0, 1]
    hist = step_both(r, hist, inp, fp, "moving call 2", ids=inp["ids"], tab=tab)
    again = dict(inp, colour=sk.scene_colour(inp["g1"], inp["g2"], np.random.default_rng(w + h)))
    hist = step_both(r, hist, again, fp, "moving call 3", ids=inp["ids"], tab=np.zeros_like(tab))
    assert clamped_pixels(hist) > 100


def test_hostile_planes(dev):
    """NaN and +-Inf channels (the fixture's), 3e38 planted (finite: it counts as a tap and its square overflows) in what becomes Hf' and Hc'; then a call
    whose every colour is NaN after a reset: Hnf' = 0 everywhere and nothing is touched"""
    r, _ = dev
    size = (45, 37)
    w, h = size
    r.create(size)
    r.track_moments(False)
    r.temporal_demodulate(False)
    for radius in (1, 3):
        fp = fh.params(2.5, 1.0, radius)
        r.temporal_fast(fp)
        r.temporal_reset()
        hist = None
        rng = np.random.default_rng(70 + radius)
        seen = np.zeros(3, bool)
        for k in (0, 1, 2):
            inp = sk.call_inputs(size, "none", k)
            for _ in range(6):
                inp["colour"][int(rng.integers(h)), int(rng.integers(w)), int(rng.integers(3))] = (-1.0 if k else 1.0) * 3.0e38
            hist = step_both(r, hist, inp, fp, f"hostile radius {radius} call {k}")
            with np.errstate(invalid="ignore"):
                seen |= [(~np.isfinite(hist.fast[..., :3])).any(), (np.abs(hist.fast[..., :3]) > 1e37).any(), (hist.fast_length < 1).any()]
        assert seen.all()
        r.temporal_reset()
        inp = sk.call_inputs(size, "none", 0)
        inp["colour"][..., 1] = np.nan
        hist = step_both(r, None, inp, fp, f"all NaN, radius {radius}")
        assert (hist.fast_length == 0).all() and (hist.length == 0).all() and np.array_equal(bits(hist.colour), bits(inp["colour"]))


def run_plain(r, size):
    """two calls with tracking on and everything the consumers hand out, as bytes"""
    out = []
    r.create(size)
    r.track_moments(True)
    tm = hd.default_tonemapper()
    for k in (1, sk.STATIC_CALLS):
        inp = sk.call_inputs(size, "yaw", k)
        r.write_accum(inp["colour"])
        r.set_denoise_guides(inp["g0"], inp["g1"], inp["g2"])
        r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
        out.append(r.temporal_accumulate(model.params_of(inp)))
    sp = sh.params(3, min_temporal=1.5)
    out += [*r.read_temporal_history(), r.read_temporal_moments(), *r.svgf_history(sp), r.tonemap_svgf(sp, tm), r.tonemap_history(None, tm)]
    return [np.ascontiguousarray(a).view(np.uint8) for a in out]


def test_the_setting_off_changes_no_byte():
    """a context that had the setting on (and ran a call with it) and off again against one that never heard of it: the same calls, the same bytes"""
    size = (70, 45)
    a, b = HipRenderer(), HipRenderer()
    try:
        a.setup(0)
        b.setup(0)
        b.create(size)
        b.temporal_fast(b.fast_params(4.0, 2.0, 2))
        inp = sk.call_inputs(size, "yaw", 0)
        b.write_accum(inp["colour"])
        b.set_denoise_guides(inp["g0"], inp["g1"], inp["g2"])
        b.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
        b.temporal_accumulate(model.params_of(inp))
        b.temporal_fast(None)
        for x, y in zip(run_plain(a, size), run_plain(b, size)):
            assert np.array_equal(x, y)
    finally:
        a.destroy()
        b.destroy()


def test_refusals_leave_the_histories_untouched_and_the_state_is_kept():
    L = capi.lib()
    size = (45, 37)
    w, h = size
    first, second = (sk.call_inputs(size, "yaw", k) for k in (0, 1))
    p = model.params_of(second)
    out, length = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32)
    fp = model.fast_params()
    r = HipRenderer()
    r.setup(0)
    try:
        err = lambda: L.pt_last_error(r._ctx)   # noqa: E731
        bad = [(fh.params(0.5, 1.0, 2), b"pt_temporal_fast: maxFast must be at least 1 and finite"), (fh.params(np.nan, 1.0, 2), b"maxFast must be"),
               (fh.params(4.0, -1.0, 2), b"pt_temporal_fast: sigmaScale must be non-negative and finite"), (fh.params(4.0, np.inf, 2), b"sigmaScale must be"),
               (fh.params(4.0, 1.0, 0), b"pt_temporal_fast: radius must be 1, 2 or 3"), (fh.params(4.0, 1.0, 4), b"radius must be"),
               (fh.params(4.0, 1.0, 2, 1), b"pt_temporal_fast: unknown flag bits")]
        for q, text in bad:
            assert L.pt_temporal_fast(r._ctx, C.byref(q)) == capi.PT_ERR_INVALID and text in err()
        assert L.pt_temporal_fast(None, C.byref(fp)) == capi.PT_ERR_INVALID
        r.create(size)
        assert L.pt_read_temporal_fast(r._ctx, out.ctypes.data, length.ctypes.data) == capi.PT_ERR_STATE and b"pt_read_temporal_fast: there is no history" in err()
        # a history made with the setting off (the refused parameters above left it off) has no fast images
        r.write_accum(first["colour"])
        r.set_denoise_guides(first["g0"], first["g1"], first["g2"])
        r.set_camera(camera_words((first["viewInverse"], first["projInverse"])))
        plain = r.temporal_accumulate(p)
        assert np.array_equal(bits(plain), bits(first["colour"]))
        assert L.pt_read_temporal_fast(r._ctx, out.ctypes.data, length.ctypes.data) == capi.PT_ERR_STATE and b"the history was made with pt_temporal_fast off" in err()
        assert not out.any() and not length.any()
        # off -> on drops the history
        r.temporal_fast(fp)
        assert L.pt_read_temporal_history(r._ctx, out.ctypes.data, None) == capi.PT_ERR_STATE and b"no history" in err()
        hist = None
        for inp in (first, second):
            hist = step_both(r, hist, inp, fp, "setup")
        before = (*r.read_temporal_history(), *r.read_temporal_fast())
        # refused parameters, and a step refused for its own reasons: nothing launched, every history as it was, the setting as it was
        for q, _ in bad:
            assert L.pt_temporal_fast(r._ctx, C.byref(q)) == capi.PT_ERR_INVALID
        r.set_denoise_guides(second["g0"], None, second["g2"])
        r.write_accum(first["colour"])
        for call in (L.pt_temporal_accumulate, L.pt_temporal_accumulate_moving):
            assert call(r._ctx, C.byref(p), out.ctypes.data) == capi.PT_ERR_STATE and b"guide planes 1 (normal) and 2 (depth)" in err()
        r.set_denoise_guides(second["g0"], second["g1"], second["g2"])
        wrong = model.params_of(second, 0.5)
        assert L.pt_temporal_accumulate(r._ctx, C.byref(wrong), out.ctypes.data) == capi.PT_ERR_INVALID
        assert not out.any()
        for x, y in zip(before, (*r.read_temporal_history(), *r.read_temporal_fast())):
            assert np.array_equal(bits(x), bits(y))
        # new parameters while the setting stays on keep the history, and the next call uses them
        wider = fh.params(3.0, 2.0, 3)
        r.temporal_fast(wider)
        assert np.array_equal(bits(r.read_temporal_fast()[0]), bits(before[2]))
        third = sk.call_inputs(size, "yaw", 2)
        hist = step_both(r, hist, third, wider, "new parameters")
        # the setting survives pt_resize (which drops the history with the images) and is independent of the other two
        r.create((64, 48))
        assert L.pt_read_temporal_fast(r._ctx, None, None) == capi.PT_ERR_STATE
        small = sk.call_inputs((64, 48), "none", 0)
        step_both(r, None, small, wider, "after pt_resize")
        r.track_moments(True)
        r.temporal_demodulate(True)
        assert L.pt_read_temporal_fast(r._ctx, None, None) == capi.PT_ERR_STATE       # (each of those changes dropped the history)
        small = ak.call_inputs((64, 48), "none", 0)
        step_both(r, None, small, wider, "with the other two settings", moments=True, demod=True)
        # on -> off drops the history
        r.temporal_fast(None)
        assert L.pt_read_temporal_history(r._ctx, out.ctypes.data, None) == capi.PT_ERR_STATE and b"no history" in err()
    finally:
        r.destroy()


def test_the_timing_entry_times_both_parts(dev):
    r, _ = dev
    L = capi.lib()
    size = (70, 45)
    r.create(size)
    r.track_moments(False)
    r.temporal_demodulate(False)
    fp = model.fast_params()
    r.temporal_fast(fp)
    r.temporal_reset()
    inp = sk.call_inputs(size, "none", 0)
    p = model.params_of(inp)
    ms = C.c_float(-1.0)
    r.write_accum(inp["colour"])
    r.set_denoise_guides(inp["g0"], inp["g1"], inp["g2"])
    r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
    assert L.pt_debug_fast_time(r._ctx, C.byref(p), 0, 2, C.byref(ms)) == capi.PT_ERR_STATE and b"there is no history" in L.pt_last_error(r._ctx)
    hist = step_both(r, None, inp, fp, "timing setup")
    before = (*r.read_temporal_history(), *r.read_temporal_fast())
    for what in (0, 1):
        ms.value = -1.0
        assert L.pt_debug_fast_time(r._ctx, C.byref(p), what, 2, C.byref(ms)) == capi.PT_OK, L.pt_last_error(r._ctx)
        assert ms.value > 0.0
    for x, y in zip(before, (*r.read_temporal_history(), *r.read_temporal_fast())):       # every run writes the set that is not the history
        assert np.array_equal(bits(x), bits(y))
    step_both(r, hist, sk.call_inputs(size, "none", 1), fp, "a call after the timing")
    assert L.pt_debug_fast_time(r._ctx, C.byref(p), 2, 2, C.byref(ms)) == capi.PT_ERR_INVALID
    assert L.pt_debug_fast_time(r._ctx, C.byref(p), 0, 0, C.byref(ms)) == capi.PT_ERR_INVALID
    r.temporal_fast(None)
    assert L.pt_debug_fast_time(r._ctx, C.byref(p), 0, 2, C.byref(ms)) == capi.PT_ERR_STATE
