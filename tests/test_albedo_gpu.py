"""The demodulated history on the device (pt_temporal_demodulate) against the host build of the same headers
(tests/albedo_host.py), which tests/test_albedo_model.py holds to the parent's host builds and to the float64 model: device == host bit for bit on every
pixel of the returned image, the history colour, the length plane and, with tracking on, the moments, for all four combinations of (moments, moving), over
a first call, a static call and the move; through the consumers (pt_svgf_history for 1 .. 5 iterations, pt_denoise_history, the two display entries); the
setting off changes no byte; the refusals leave the history untouched; the state the context keeps; the timing entry."""
import ctypes as C

import numpy as np
import pytest

from tests import albedo_host as ah, denoise_host as dh, motion_host as mh, svgf_host as sh
from tests import test_albedo_model as model
from tests.test_motion_gpu import identity_worlds, node_array, three_node_scene, words_of
from tests.test_temporal_gpu import camera_words
from vk_raytrace_amd import capi, host_device as hd
from vk_raytrace_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu
ak, sk, tk, bits = model.ak, model.sk, model.tk, model.bits

# tile edges of the 32 x 8 and 32 x 16 blocks, a lone pixel, a column narrower than a wave row
SIZES = [(70, 45), (45, 37), (1, 1), (3, 200), (129, 17)]


@pytest.fixture(scope="module")
def dev():
    r = HipRenderer()
    r.setup(0)
    sc = three_node_scene()
    r.set_scene(sc)
    yield r, sc
    r.temporal_demodulate(False)
    r.track_moments(False)
    r.destroy()


def same(a, b, what):
    diff = bits(a) != bits(b)
    assert not diff.any(), f"{what}: {int(diff.sum())} words differ from the host build"


def sequence_inputs(size, move):
    """a first call, a static call, the move"""
    return [ak.call_inputs(size, move, k) for k in (0, 1, sk.STATIC_CALLS)]


def step_both(r, hist, inp, moments, what, ids=None, tab=None):
    """one call of the demodulating step on the device and on the host build from the host's history (which the device's has equalled so far); ids: the
    moving form, with the table the host build takes"""
    r.write_accum(inp["colour"])
    r.set_denoise_guides(inp["g0"], inp["g1"], inp["g2"])
    r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
    p = model.params_of(inp)
    if ids is None:
        got = r.temporal_accumulate(p)
    else:
        r.set_instance_plane(ids)
        got = r.temporal_accumulate_moving(p)
    rc, want = ah.temporal(inp["colour"], inp["g0"], inp["g1"], inp["g2"], inp["viewInverse"], inp["projInverse"], p, hist, moments=moments, ids=ids, tab=tab)
    assert rc == 0
    hc, hn = r.read_temporal_history()
    same(got, want.colour, f"{what}: returned image")
    same(hc, want.colour, f"{what}: history colour")
    same(hn, want.length, f"{what}: history length")
    if moments:
        same(r.read_temporal_moments(), want.moments, f"{what}: moments")
    return want


def consumers_both(r, hist, inp, moments, what, iterations=(1, 2, 3, 4, 5)):
    """the remodulating consumers of the history `hist` (the host's, which the device's equals) against the host build, and the display entries against
    pt_tonemap of their float result"""
    guides = (inp["g0"], inp["g1"], inp["g2"])
    tm = hd.default_tonemapper()
    dp = dh.params(3, 0.5, (1e15, 0.3, 0.5))
    rc, filtered = dh.denoise(hist.colour, guides, dp)
    assert rc == 0
    want = ah.remodulate(filtered, inp["g0"])
    got = r.denoise_history(dp)
    same(got, want, f"{what}: pt_denoise_history")
    shown, shown_plain = r.tonemap_history(dp, tm), r.tonemap_history(None, tm)
    r.write_accum(got)
    assert np.array_equal(shown, r.tonemap(tm)), f"{what}: pt_tonemap_history"
    r.write_accum(ah.remodulate(hist.colour, inp["g0"]))
    assert np.array_equal(shown_plain, r.tonemap(tm)), f"{what}: pt_tonemap_history without a filter"
    if not moments:
        return
    for n in iterations:
        sp = sh.params(n, sigma_guide=(1e15, 0.3, 0.5), min_temporal=1.5)
        rc, img, var = ah.svgf_history(hist, guides, sp)
        assert rc == 0
        c, v = r.svgf_history(sp)
        same(c, img, f"{what}: pt_svgf_history after {n} iterations")
        same(v, var, f"{what}: variance after {n} iterations (demodulated units)")
    shown = r.tonemap_svgf(sp, tm)
    r.write_accum(c)
    assert np.array_equal(shown, r.tonemap(tm)), f"{what}: pt_tonemap_svgf"
    rc, v0 = sh.variance(hist.colour, hist.length, hist.moments, guides, sp)
    same(r.svgf_variance(sp), v0, f"{what}: V0 (demodulated units)")


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_host_build_bit_for_bit(dev, size, moments):
    """the static form: a first call, a static call and the move, then the consumers of what that leaves"""
    r, _ = dev
    w, h = size
    r.create(size)
    r.track_moments(moments)
    r.temporal_demodulate(True)
    for move in ("yaw", "disocclude"):
        r.temporal_reset()
        hist = None
        for k, inp in enumerate(sequence_inputs(size, move)):
            hist = step_both(r, hist, inp, moments, f"{w}x{h} {move} call {k + 1}")
            if k == 0 and move == "yaw":
                consumers_both(r, hist, inp, moments, f"{w}x{h} {move} after the first call", iterations=(1,))
        consumers_both(r, hist, inp, moments, f"{w}x{h} {move}", iterations=(1, 2, 3, 4, 5) if move == "yaw" else (5,))


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
def test_the_moving_form_equals_the_host_build_bit_for_bit(dev, moments):
    """70 x 45, one moved instance: a first call with the box where the history has it, pt_update_instances and the move, a call after it"""
    r, sc = dev
    size = (70, 45)
    w, h = size
    r.create(size)
    r.track_moments(moments)
    r.temporal_demodulate(True)
    for move in ("slide", "yaw"):
        r.temporal_reset()
        inp = ak.motion_inputs(size, move)
        H = inp["hist"]
        start = tk.moved("none", w / h)
        g2_0 = np.zeros((h, w, 4), np.float32)
        g1_0 = H["guide"].copy()
        g1_0[..., 3], g2_0[..., 0] = 1.0, H["guide"][..., 3]
        first = dict(inp, colour=H["colour"], g1=g1_0, g2=g2_0, viewInverse=start["viewInverse"], projInverse=start["projInverse"], worldToClip=start["worldToClip"])
        r.update_instances(node_array(sc, identity_worlds()))
        hist = step_both(r, None, first, moments, f"{move} call 1", ids=H["ids"])
        words = words_of(identity_worlds())
        worlds = identity_worlds(inp["box"])
        r.update_instances(node_array(sc, worlds))
        tab = mh.table(words, words_of(worlds))
        assert mh.moved_bits(tab).tolist() == [0, 0, 1]
        hist = step_both(r, hist, inp, moments, f"{move} call 2", ids=inp["ids"], tab=tab)
        again = dict(inp, colour=tk.noisy_colour(w, h, np.random.default_rng(w + h)))
        hist = step_both(r, hist, again, moments, f"{move} call 3", ids=inp["ids"], tab=np.zeros_like(tab))
    consumers_both(r, hist, again, moments, "moving", iterations=(3,))


def run_plain(r, size):
    """two calls with tracking on and everything the consumers hand out, as bytes"""
    out = []
    r.create(size)
    r.track_moments(True)
    tm = hd.default_tonemapper()
    for inp in sequence_inputs(size, "yaw")[1:]:
        r.write_accum(inp["colour"])
        r.set_denoise_guides(inp["g0"], inp["g1"], inp["g2"])
        r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
        out.append(r.temporal_accumulate(model.params_of(inp)))
    sp, dp = sh.params(3, min_temporal=1.5), dh.params(2, 0.5, (0.5, 0.3, 0.5), capi.PT_DENOISE_DEMODULATE)
    out += [*r.read_temporal_history(), r.read_temporal_moments(), *r.svgf_history(sp), r.tonemap_svgf(sp, tm), r.denoise_history(dp), r.tonemap_history(dp, tm),
            r.tonemap_history(None, tm)]
    return [np.ascontiguousarray(a).view(np.uint8) for a in out]


def test_the_setting_off_changes_no_byte():
    """a context that had the setting on and off again against one that never heard of it: the same calls, the same bytes"""
    size = (70, 45)
    a, b = HipRenderer(), HipRenderer()
    try:
        a.setup(0)
        b.setup(0)
        b.temporal_demodulate(True)
        b.temporal_demodulate(False)
        for x, y in zip(run_plain(a, size), run_plain(b, size)):
            assert np.array_equal(x, y)
    finally:
        a.destroy()
        b.destroy()


def test_refusals_leave_the_history_untouched_and_the_state_is_kept():
    L = capi.lib()
    size = (45, 37)
    w, h = size
    first, second = sequence_inputs(size, "yaw")[:2]
    p = model.params_of(second)
    tm = hd.default_tonemapper()
    sp, dp = sh.params(2, min_temporal=1.5), dh.params(2, 0.5)
    dpd = dh.params(2, 0.5, flags=capi.PT_DENOISE_DEMODULATE)
    out, rgba = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.uint8)
    r = HipRenderer()
    r.setup(0)
    try:
        err = lambda: L.pt_last_error(r._ctx)   # noqa: E731
        for bad in (2, -1, 256):
            assert L.pt_temporal_demodulate(r._ctx, bad) == capi.PT_ERR_INVALID and b"pt_temporal_demodulate: on must be 0 or 1" in err()
        assert L.pt_temporal_demodulate(None, 1) == capi.PT_ERR_INVALID
        r.create(size)
        r.track_moments(True)
        r.temporal_demodulate(True)
        hist = None
        for inp in (first, second):
            hist = step_both(r, hist, inp, True, "setup")
        before = (*r.read_temporal_history(), r.read_temporal_moments())
        # plane 0 missing: at the step, with its own text, and at each consumer, with the one text they share
        r.set_denoise_guides(None, second["g1"], second["g2"])
        r.write_accum(first["colour"])
        for call in (L.pt_temporal_accumulate, L.pt_temporal_accumulate_moving):
            assert call(r._ctx, C.byref(p), out.ctypes.data) == capi.PT_ERR_STATE and b"pt_temporal_demodulate is on: guide plane 0" in err()
        consumers = [("pt_svgf_history", lambda: L.pt_svgf_history(r._ctx, C.byref(sp), out.ctypes.data, None)),
                     ("pt_tonemap_svgf", lambda: L.pt_tonemap_svgf(r._ctx, C.byref(sp), C.byref(tm), rgba.ctypes.data)),
                     ("pt_denoise_history", lambda: L.pt_denoise_history(r._ctx, C.byref(dp), out.ctypes.data)),
                     ("pt_tonemap_history", lambda: L.pt_tonemap_history(r._ctx, C.byref(dp), C.byref(tm), rgba.ctypes.data)),
                     ("pt_tonemap_history", lambda: L.pt_tonemap_history(r._ctx, None, C.byref(tm), rgba.ctypes.data))]
        for name, call in consumers:
            assert call() == capi.PT_ERR_STATE, name
            assert err().startswith(name.encode() + b": the history is demodulated (pt_temporal_demodulate): guide plane 0"), err()
        assert not out.any() and not rgba.any()
        # the variance alone multiplies nothing and needs no plane
        assert L.pt_svgf_variance(r._ctx, C.byref(sp), out[..., 0].copy().ctypes.data) == capi.PT_OK
        r.set_denoise_guides(second["g0"], second["g1"], second["g2"])
        for call in (lambda: L.pt_denoise_history(r._ctx, C.byref(dpd), out.ctypes.data), lambda: L.pt_tonemap_history(r._ctx, C.byref(dpd), C.byref(tm), rgba.ctypes.data)):
            assert call() == capi.PT_ERR_STATE and b"already demodulated" in err()
        after = (*r.read_temporal_history(), r.read_temporal_moments())
        for x, y in zip(before, after):
            assert np.array_equal(bits(x), bits(y))
        for name, call in consumers:
            assert call() == capi.PT_OK, (name, err())
        # the same value again keeps the history; tracking is independent of the setting; a change drops the history as pt_temporal_reset does
        r.temporal_demodulate(True)
        assert np.array_equal(bits(r.read_temporal_history()[0]), bits(before[0]))
        r.temporal_demodulate(False)
        assert L.pt_read_temporal_history(r._ctx, out.ctypes.data, None) == capi.PT_ERR_STATE and b"no history" in err()
        r.write_accum(first["colour"])
        got = r.temporal_accumulate(p)
        assert np.array_equal(bits(got), bits(first["colour"]))                              # a first call, undemodulated
        assert np.array_equal(bits(r.denoise_history(dpd)), bits(r.denoise_history(dpd)))    # ... whose consumers take PT_DENOISE_DEMODULATE again
        r.temporal_demodulate(True)
        assert L.pt_read_temporal_history(r._ctx, out.ctypes.data, None) == capi.PT_ERR_STATE
        got = r.temporal_accumulate(p)
        assert np.array_equal(bits(got), bits(ak.dk.demodulate(first["colour"], second["g0"])))   # a first call stores the quotient
        # pt_resize keeps the setting (and drops the planes with the history)
        r.create((64, 48))
        small = ak.call_inputs((64, 48), "none", 0)
        r.write_accum(small["colour"])
        r.set_camera(camera_words((small["viewInverse"], small["projInverse"])))
        r.set_denoise_guides(None, small["g1"], small["g2"])
        assert L.pt_temporal_accumulate(r._ctx, C.byref(model.params_of(small)), None) == capi.PT_ERR_STATE and b"pt_temporal_demodulate is on" in err()
        r.set_denoise_guides(small["g0"], small["g1"], small["g2"])
        got = r.temporal_accumulate(model.params_of(small))
        assert np.array_equal(bits(got), bits(ak.dk.demodulate(small["colour"], small["g0"])))
        assert r.read_temporal_moments().shape == (48, 64, 2)                                     # tracking survived as well
    finally:
        r.destroy()


def test_the_timing_entry_times_both_parts(dev):
    r, _ = dev
    L = capi.lib()
    size = (70, 45)
    r.create(size)
    r.track_moments(True)
    r.temporal_demodulate(True)
    r.temporal_reset()
    inp = ak.call_inputs(size, "none", 0)
    step_both(r, None, inp, True, "timing setup")
    p = model.params_of(inp)
    ms = C.c_float(-1.0)
    before = r.read_temporal_history()
    for what in (0, 1):
        ms.value = -1.0
        assert L.pt_debug_albedo_time(r._ctx, C.byref(p), what, 2, C.byref(ms)) == capi.PT_OK, L.pt_last_error(r._ctx)
        assert ms.value > 0.0
    for x, y in zip(before, r.read_temporal_history()):       # every run reads the history and writes the other set
        assert np.array_equal(bits(x), bits(y))
    assert L.pt_debug_albedo_time(r._ctx, C.byref(p), 2, 2, C.byref(ms)) == capi.PT_ERR_INVALID
    assert L.pt_debug_albedo_time(r._ctx, C.byref(p), 0, 0, C.byref(ms)) == capi.PT_ERR_INVALID
    r.temporal_demodulate(False)
    assert L.pt_debug_albedo_time(r._ctx, C.byref(p), 0, 2, C.byref(ms)) == capi.PT_ERR_STATE
    r.temporal_demodulate(True)
