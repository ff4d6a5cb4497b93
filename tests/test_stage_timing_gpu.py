"""The device-event timing entries of the four display stages (pt_debug_denoise_time, pt_debug_temporal_time, pt_debug_svgf_time, pt_debug_guides_time:
csrc/pt_stage.h's stage_time under each of them), which only the rate tools under tools/ call otherwise: every part they can time returns PT_OK and a finite
positive figure, their argument and state errors carry the entry's own name, and what they promise to leave alone -- the history, the moments, the filter's
result, the guide planes -- holds the same bits afterwards.  70 x 45: two tiles and a ragged edge in both directions for every stage's tile; reps = 2."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import test_svgf_model as model
from tests.test_guides_gpu import opaque_scene, open_renderer
from tests.test_svgf_gpu import sequence_inputs
from tests.test_temporal_gpu import camera_words
from vk_raytrace_amd import capi, host_device as hd
from vk_raytrace_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu
bits = model.bits
SIZE, REPS, MISS_DEPTH = (70, 45), 2, 50.0
SIGMA_GUIDE = (1.0, 0.3, 0.5)


@pytest.fixture(scope="module")
def dev():
    r = HipRenderer()
    r.setup(0)
    yield r
    r.destroy()


def denoise_params(n):
    return hd.DenoiseParams(iterations=n, sigmaColor=1.0, sigmaGuide=SIGMA_GUIDE, flags=0)


def install(r, inp):
    r.write_accum(inp["colour"])
    r.set_denoise_guides(inp["g0"], inp["g1"], inp["g2"])
    r.set_camera(camera_words((inp["viewInverse"], inp["projInverse"])))
    return model.temporal_params(inp)


def with_history(r, on, move="disocclude"):
    """two calls of the move (both buffer sets written), then the inputs of the third installed: its params"""
    first, second, third = sequence_inputs(SIZE, move)
    r.create(SIZE)
    r.track_moments(on)
    r.temporal_reset()
    for inp in (first, second):
        r.temporal_accumulate(install(r, inp), read=False)
    return install(r, third)


def timed(r, name, *args, reps=REPS):
    """one timing entry: PT_OK and a finite, positive time per run"""
    ms = C.c_float(-1.0)
    r._check(getattr(capi.lib(), name)(r._ctx, *args, reps, C.byref(ms)))
    assert math.isfinite(ms.value) and ms.value > 0.0, (name, ms.value)
    return ms.value


def held(r, moments):
    hc, hn = r.read_temporal_history()
    return [bits(hc), bits(hn)] + ([bits(r.read_temporal_moments())] if moments else [])


def assert_same(before, after, what):
    assert len(before) == len(after)
    for k, (a, b) in enumerate(zip(before, after)):
        assert np.array_equal(a, b), f"{what}: item {k} changed"


@pytest.mark.parametrize("iterations", [1, 3])
def test_denoise_time(dev, iterations):
    dev.create(SIZE)
    install(dev, sequence_inputs(SIZE, "yaw")[0])
    p = denoise_params(iterations)
    before = bits(dev.denoise(p))
    timed(dev, "pt_debug_denoise_time", C.byref(p))
    assert np.array_equal(bits(dev.denoise(p)), before)


@pytest.mark.parametrize("on", [False, True], ids=["tracking-off", "tracking-on"])
def test_temporal_time_leaves_the_history_as_it_was(dev, on):
    p = with_history(dev, on)
    before = held(dev, on)
    timed(dev, "pt_debug_temporal_time", C.byref(p))
    assert_same(before, held(dev, on), "pt_debug_temporal_time")
    dev.temporal_reset()          # a first call (no history) is timed as well
    timed(dev, "pt_debug_temporal_time", C.byref(p))
    assert capi.lib().pt_read_temporal_history(dev._ctx, None, None) == capi.PT_ERR_STATE


@pytest.mark.parametrize("what", [-2, -1, 0, 3], ids=["whole", "variance", "first", "last"])
def test_svgf_time_leaves_the_history_and_the_result_as_they_were(dev, what):
    with_history(dev, True)
    p = dev.svgf_params(4, sigma_guide=SIGMA_GUIDE, min_temporal=2.5)
    assert what == p.iterations - 1 or what < 1
    before, shown = held(dev, True), [bits(x) for x in dev.svgf_history(p)]
    timed(dev, "pt_debug_svgf_time", C.byref(p), what)
    assert_same(before, held(dev, True), "pt_debug_svgf_time")
    assert_same(shown, [bits(x) for x in dev.svgf_history(p)], "pt_svgf_history after pt_debug_svgf_time")


@pytest.mark.parametrize("accel", [capi.PT_ACCEL_FLAT, capi.PT_ACCEL_TWO_LEVEL], ids=["flat", "two-level"])
def test_guides_time_leaves_the_planes_of_the_pass(accel):
    r = open_renderer(opaque_scene(), SIZE, accel=accel)
    try:
        r.capture_guides(7, MISS_DEPTH)
        want = r.read_guides()
        r.set_denoise_guides(None, None, None)
        timed(r, "pt_debug_guides_time", 7, MISS_DEPTH)
        for j, (a, b) in enumerate(zip(r.read_guides(), want)):
            assert np.array_equal(bits(a), bits(b)), f"plane {j}"
    finally:
        r.destroy()


def test_errors_carry_the_entry_name():
    L = capi.lib()
    ms = C.c_float(-1.0)
    dp, sp = denoise_params(2), HipRenderer.svgf_params(3, sigma_guide=SIGMA_GUIDE, min_temporal=2.5)
    r = open_renderer(opaque_scene())
    try:
        tp = model.temporal_params(sequence_inputs(SIZE, "yaw")[0])

        def entries(reps, out):
            return (("pt_debug_denoise_time", lambda: L.pt_debug_denoise_time(r._ctx, C.byref(dp), reps, out)),
                    ("pt_debug_temporal_time", lambda: L.pt_debug_temporal_time(r._ctx, C.byref(tp), reps, out)),
                    ("pt_debug_svgf_time", lambda: L.pt_debug_svgf_time(r._ctx, C.byref(sp), -2, reps, out)),
                    ("pt_debug_guides_time", lambda: L.pt_debug_guides_time(r._ctx, 7, MISS_DEPTH, reps, out)))

        def refused(code, reps=REPS, out=C.byref(ms), only=None, says=None):
            for name, call in entries(reps, out):
                if only is None or name in only:
                    assert call() == code, name
                    err = L.pt_last_error(r._ctx)
                    assert err.startswith(name.encode()), (name, err)
                    assert says is None or says in err, (name, err)

        # before pt_resize (the guide pass names what it misses first: the camera)
        refused(capi.PT_ERR_STATE, only=("pt_debug_denoise_time", "pt_debug_temporal_time", "pt_debug_svgf_time"), says=b"before pt_resize")
        refused(capi.PT_ERR_STATE, only=("pt_debug_guides_time",))
        # reps = 0 and a null ms_out, in any state
        refused(capi.PT_ERR_INVALID, reps=0)
        refused(capi.PT_ERR_INVALID, out=None)
        with_history(r, False)
        refused(capi.PT_ERR_INVALID, reps=0)
        refused(capi.PT_ERR_INVALID, out=None)
        # the filter's timing without a history with moments
        refused(capi.PT_ERR_STATE, only=("pt_debug_svgf_time",), says=b"without moments")
        r.temporal_reset()
        refused(capi.PT_ERR_STATE, only=("pt_debug_svgf_time",), says=b"no history")
        with_history(r, True)
        for what in (-3, sp.iterations):
            assert L.pt_debug_svgf_time(r._ctx, C.byref(sp), what, REPS, C.byref(ms)) == capi.PT_ERR_INVALID, what
            assert L.pt_last_error(r._ctx).startswith(b"pt_debug_svgf_time"), what
        assert ms.value == -1.0          # no refused call wrote a figure
        assert L.pt_debug_svgf_time(r._ctx, C.byref(sp), sp.iterations - 1, REPS, C.byref(ms)) == capi.PT_OK and ms.value > 0.0
        assert L.pt_debug_denoise_time(None, C.byref(dp), REPS, C.byref(ms)) == capi.PT_ERR_INVALID
    finally:
        r.destroy()
